"""CPU-side checks of RSA-2048 signing: the golden fixture against the oracle, the signing entries
of the C ABI and the Python binding, and the kernels' CRT scheme restated on Python integers."""
import os
import re

import pytest

import cbft_hipcrypto as cb
import rsa_ref
import rsagen
from rsa_sign_vectors import (LENGTHS, PATH, crt_edge_ems, crt_params, crt_sign, em_of, load_rsa_sign_vectors)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGN_SYMBOLS = ["cbft_rsa_load_signers", "cbft_rsa_signer_status", "cbft_rsa_signer_moduli",
                "cbft_rsa_unload_signers", "cbft_rsa_sign_batch", "cbft_rsa_sign_fixed_device"]
METHODS = ["rsa_load_signers", "rsa_signer_status", "rsa_signer_moduli", "rsa_unload_signers", "rsa_sign_batch",
           "rsa_sign_fixed_device"]


@pytest.fixture(scope="module")
def vectors():
    return load_rsa_sign_vectors()


@pytest.fixture(scope="module")
def keys():
    return rsagen.load_keys()


def test_fixture_parses(vectors, keys):
    assert os.path.getsize(PATH) < 200_000
    assert len(vectors) == 8 * len(LENGTHS) + 1
    for ki in range(8):
        assert [len(v.msg) for v in vectors[:-1] if v.key == ki] == LENGTHS
    assert len(vectors[-1].msg) == 4096
    assert all(len(v.sig) == 256 for v in vectors)
    assert sorted({k["e"] for k in keys}) == [3, 17, 65537, 0xC0000001]
    assert {k["p"] > k["q"] for k in keys} == {True, False}  # both prime orders
    assert sum(k["p"] < k["q"] for k in keys) == 3


def test_every_vector_equals_the_oracle_and_verifies(vectors, keys):
    for i, v in enumerate(vectors):
        k = keys[v.key]
        assert rsa_ref.sign(k["n"], k["d"], v.msg) == v.sig, i
        assert rsa_ref.verify(k["n"], k["e"], v.msg, v.sig), i


def test_header_declares_the_signing_entries():
    src = open(os.path.join(ROOT, "include", "cbft_hipcrypto.h")).read()
    declared = set(re.findall(r"\b(cbft_[a-z0-9_]+)\s*\(", src))
    for s in SIGN_SYMBOLS:
        assert s in declared, s
        assert s in {n for n, _, _ in cb.ABI}, s
    assert "CBFT_RSA_SIGN_GPU_MIN" in src  # listed in the environment block


def test_binding_has_the_signing_methods():
    for m in METHODS:
        assert callable(getattr(cb.Context, m, None)), m


def test_library_exports_the_signing_entries():
    assert os.path.exists(cb.LIB_PATH), "libcbft_hipcrypto.so not built"
    lib = cb.load_library()
    for s in SIGN_SYMBOLS:
        assert hasattr(lib, s), s


def test_crt_restatement_equals_pow_on_the_fixture(vectors, keys):
    for v in vectors:
        k = keys[v.key]
        p, q, dP, dQ, qInv, _ = crt_params(k)
        s = crt_sign(em_of(v.msg), p, q, dP, dQ, qInv)
        assert s == pow(em_of(v.msg), k["d"], k["n"])
        assert s.to_bytes(256, "big") == v.sig


def test_crt_restatement_on_the_arithmetic_edges(keys):
    """EM = 0, 1, n - 1, multiples of either prime, m_p == m_q, m_p < m_q, m_q >= p: for every
    fixture key, so for both prime orders."""
    seen = set()
    for k in keys:
        p, q, dP, dQ, qInv, _ = crt_params(k)
        edges = crt_edge_ems(p, q, dP, dQ, qInv)
        assert ("mq_ge_p" in edges) == (p < q)
        for name, em in edges.items():
            assert 0 <= em < k["n"]
            assert crt_sign(em, p, q, dP, dQ, qInv) == pow(em, k["d"], k["n"]), (name, k["e"])
            seen.add(name)
        assert (pow(edges["mp_lt_mq"], dP, p), pow(edges["mp_lt_mq"], dQ, q)) == (5, 7)
        assert pow(edges["mp_eq_mq"], dP, p) == pow(edges["mp_eq_mq"], dQ, q) == 12345
        if "mq_ge_p" in edges:
            assert pow(edges["mq_ge_p"], dQ, q) >= p
    assert seen == {"zero", "one", "n_minus_1", "multiple_of_p", "multiple_of_q", "mp_eq_mq", "mp_lt_mq", "mq_ge_p"}
