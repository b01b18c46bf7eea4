"""CPU tests of batched BLS key derivation and dealing: the lane routines of csrc/bls_keygen_batch.h (the
source the GPU runs one key, coefficient or share per lane) built for the host
(tests/cpp/bls_keygen_shim.cpp), against the golden fixture the Python oracle wrote
(tests/golden/bls_keygen_vectors.json), the plain double-and-add of the branching host code and Python
integers."""
import ctypes
import os
import random
import subprocess

import pytest

import bn254_ref as B
from bls_keygen_vectors import (HERE, PATH, R, ZERO65, dump_fixture, horner, keygen_shim, lane_deal, lane_keys,
                                lane_reduce, load_fixture, plain_keys, recoded_nibbles)


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def test_fixture_covers_the_edges(fixture):
    sks = {v.sk for v in fixture}
    assert {1, 2, 3, R - 1, R - 2, 0, R, R + 1, 2 * R - 1, 2**255, 2**256 - 1} <= sks
    assert any(s % 2 == 0 and s + 1 in sks for s in sks if 3 < s < R - 3), "no even / odd neighbour pair"
    assert all((v.ok == 0) == (v.sk % R == 0) and (v.vk == ZERO65) == (v.ok == 0) for v in fixture)
    # every table entry and both signs at every position: nibble v at position j for all v, j <= 62
    seen = set()
    for v in fixture:
        if v.ok:
            seen |= {(j, nib) for j, nib in enumerate(recoded_nibbles(v.sk))}
    assert {(j, nib) for j in range(63) for nib in range(16)} <= seen
    assert {(63, 8), (63, 9)} <= seen
    assert any(v.ok and v.sk % R % 2 == 0 for v in fixture) and len(fixture) >= 64
    assert R == B.R


def test_fixture_loader_round_trips(fixture, tmp_path):
    p = tmp_path / "copy.json"
    dump_fixture(str(p), fixture)
    assert p.read_bytes() == open(PATH, "rb").read()
    assert load_fixture(str(p)) == fixture


def test_fixture_is_the_oracle(fixture):
    """Four fixture keys, recomputed with the oracle here (the generator wrote all of them the same way)."""
    for v in [v for v in fixture if v.ok][:4]:
        assert B.g2_to_bytes(B.ec_mul(v.sk % R, B.G2_GEN)) == v.vk, v.cls


def test_whole_fixture_through_the_lane_routine(fixture):
    """Every key byte for byte through the host build of bls_keygen_lane, against the oracle's bytes in the
    fixture and against the plain double-and-add."""
    got, ok = lane_keys([v.sk for v in fixture])
    bad = [i for i, v in enumerate(fixture) if got[i] != v.vk or ok[i] != v.ok]
    assert not bad, f"{len(bad)} keys differ from the fixture, first {[fixture[i].cls for i in bad[:8]]}"
    assert got == plain_keys([v.sk for v in fixture])


def test_random_scalars_against_double_and_add():
    rng = random.Random(41)
    sks = [rng.randrange(2**256) for _ in range(192)] + [rng.randrange(1, 2**64) for _ in range(32)]
    got, ok = lane_keys(sks)
    assert got == plain_keys(sks) and ok.tolist() == [1] * len(sks)


def test_fp2_ct_forms_equal_the_branching_forms():
    """fp2 add / sub / neg / mul / sqr on f_add_ct / f_sub_ct == the branching forms limb for limb: random
    pairs, and the top-limb ties in both components where the signed pass ends negative."""
    lib = keygen_shim()
    fixed = ctypes.c_long()
    assert lib.bls_keygen_shim_fp2_random(ctypes.c_uint64(7), ctypes.c_long(50000), ctypes.byref(fixed)) == 0
    assert lib.bls_keygen_shim_fp2_ties(ctypes.c_uint64(8), ctypes.c_long(4000), ctypes.byref(fixed)) == 0
    assert fixed.value > 1000, "the tie cases did not reach the correction pass"


def test_reduction_mod_r():
    rng = random.Random(42)
    xs = [0, 1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 3 * R, 4 * R - 1, 4 * R, 5 * R, 6 * R - 1, 6 * R, 6 * R + 1,
          2**255, 2**256 - 1] + [rng.randrange(2**256) for _ in range(2000)]
    assert 7 * R > 2**256
    assert [lane_reduce(x) for x in xs] == [x % R for x in xs]


DEAL_CASES = [
    ("k1", [12345], 5),                          # every share is c_0
    ("k_eq_n", [7, 11, 13, 17, 19], 5),
    ("zero_share_3", [R - 3, 1], 5),             # f(3) = 0
    ("zero_secret", [0, 5, 9], 4),
    ("zero_secret_r", [R, 5, 9], 4),
    ("above_r", [R + 5, 2**256 - 1, 2**255], 6),  # the same outputs as the reductions
    ("top", [R - 1] * 4, 7),
]


@pytest.mark.parametrize("name,coeffs,n", DEAL_CASES, ids=[c[0] for c in DEAL_CASES])
def test_dealing_cases(name, coeffs, n):
    got = lane_deal(coeffs, n)
    assert got == [coeffs[0] % R] + [horner(coeffs, i) for i in range(1, n + 1)]
    assert got == lane_deal([c % R for c in coeffs], n)
    if name == "k1":
        assert got == [12345] * (n + 1)
    if name == "zero_share_3":
        assert got[3] == 0 and all(got[i] for i in (0, 1, 2, 4, 5))
    if name.startswith("zero_secret"):
        assert got[0] == 0


def test_dealing_random_k_n():
    rng = random.Random(43)
    shapes = [(1, 1), (1, 64), (64, 64), (2, 3), (22, 64), (63, 64)] + [
        (k, rng.randrange(k, 65)) for k in (rng.randrange(1, 65) for _ in range(10))]
    for k, n in shapes:
        coeffs = [rng.randrange(2**256) for _ in range(k)]
        assert lane_deal(coeffs, n) == [coeffs[0] % R] + [horner(coeffs, i) for i in range(1, n + 1)], (k, n)


def test_any_k_shares_interpolate_to_the_secret():
    rng = random.Random(44)
    for k, n in ((1, 3), (3, 5), (5, 5), (22, 64)):
        coeffs = [rng.randrange(1, R) for _ in range(k)]
        shares = lane_deal(coeffs, n)
        for _ in range(3):
            ids = sorted(rng.sample(range(1, n + 1), k))
            lam = B.lagrange_coeffs(ids)
            assert sum(lam[i] * shares[i] for i in ids) % R == coeffs[0], (k, n, ids)


def test_sanitizer_build_of_the_shim():
    """The same source as a stand-alone program under ASan + UBSan (never loaded into python)."""
    exe = os.path.join(HERE, "cpp", "bls_keygen_shim_san")
    assert os.path.exists(exe), "tests/cpp/bls_keygen_shim_san not built (make bls_keygen_shim)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
