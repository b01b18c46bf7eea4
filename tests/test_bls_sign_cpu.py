"""CPU tests of batched BLS share signing: the lane routine of csrc/bls_sign_batch.h (the source the
GPU runs one message per lane) built for the host (tests/cpp/bls_sign_shim.cpp), against the golden
fixture the Python oracle wrote (tests/golden/bls_sign_vectors.json)."""
import ctypes
import os

import numpy as np
import pytest

import bn254_ref as B
from bls_sign_vectors import PATH, dump_fixture, lane_sign_many, load_fixture, sign_shim


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def test_fixture_covers_the_edges(fixture):
    signers, vectors = fixture
    sks = {sk for sk, _ in signers}
    assert {1, 2, 3, B.R - 1, B.R - 2, 2**127 - 1, 2**127 + 1, 2**128} <= sks
    roots = [sk for sk in sks if sk != 1 and pow(sk, 3, B.R) == 1]
    assert len(roots) == 2 and all(w + 1 in sks and w - 1 in sks for w in roots)
    assert all(1 <= sid <= 2048 for _, sid in signers) and any(sid == 2048 for _, sid in signers)
    lens = {len(v.msg) for v in vectors}
    assert set(range(131)) | {1000, 4096} <= lens
    assert set(range(13)) | {16} <= {v.inc for v in vectors}
    assert len(vectors) >= 400


def test_fixture_loader_round_trips(fixture, tmp_path):
    signers, vectors = fixture
    p = tmp_path / "copy.json"
    dump_fixture(str(p), signers, vectors)
    assert p.read_bytes() == open(PATH, "rb").read()
    assert load_fixture(str(p)) == (signers, vectors)


@pytest.mark.parametrize("window", [0, 3, 4])
def test_whole_fixture_through_the_lane_routine(fixture, window):
    """Every share byte for byte, and the hash's increments, through the host build of
    bls_signer_record + bls_sign_lane: the window the product runs (0) and both built variants."""
    signers, vectors = fixture
    got, incs = lane_sign_many(signers, [v.signer for v in vectors], [v.msg for v in vectors], window=window)
    bad = [i for i, v in enumerate(vectors) if got[i].tobytes() != v.share]
    assert not bad, f"{len(bad)} shares differ, first {bad[:8]}"
    assert [int(x) for x in incs] == [v.inc for v in vectors]


def test_ct_add_sub_equal_the_branching_forms():
    """f_add_ct / f_sub_ct == f_add / f_sub limb for limb: 10^5 random pairs, and the top-limb ties
    (a8 + b8 in {T - 1, T}, a8 == b8) where the signed pass ends negative and the correction runs."""
    lib = sign_shim()
    fixed = ctypes.c_long()
    assert lib.bls_sign_shim_addsub_random(ctypes.c_uint64(5), ctypes.c_long(100000), ctypes.byref(fixed)) == 0
    assert lib.bls_sign_shim_addsub_ties(ctypes.c_uint64(6), ctypes.c_long(4000), ctypes.byref(fixed)) == 0
    assert fixed.value > 1000, "the tie cases did not reach the correction pass"


def test_fixture_shares_verify(fixture):
    """Eight fixture shares (the degenerate scalars first) pass the oracle's pairing check."""
    signers, vectors = fixture
    seen, picked = set(), []
    for v in vectors:
        if v.signer not in seen and len(picked) < 8:
            seen.add(v.signer)
            picked.append(v)
    for v in picked:
        sk, sid = signers[v.signer]
        got_id, sigma = B.parse_share(v.share)
        assert got_id == sid
        assert B.verify_share(B.g1_map(v.msg), sigma, B.ec_mul(sk, B.G2_GEN)), f"signer {v.signer}"
