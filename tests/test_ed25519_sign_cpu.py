"""CPU-side checks of Ed25519 signing: the golden fixture against the pure-Python oracle, and the
signing entries of the C ABI (declared in the header, exported by the built library)."""
import os
import re

import pytest

import cbft_hipcrypto as cb
import ed25519_ref
from sign_vectors import PATH, load_sign_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGN_SYMBOLS = ["cbft_ed25519_load_signers", "cbft_ed25519_signer_public_keys", "cbft_ed25519_unload_signers",
                "cbft_ed25519_sign_batch", "cbft_ed25519_sign_fixed_device"]
LENGTHS = [0, 1, 31, 32, 47, 48, 63, 64, 79, 80, 111, 112, 127, 128, 175, 176, 207, 208, 239, 240, 256, 1023]


@pytest.fixture(scope="module")
def vectors():
    return load_sign_vectors()


def test_fixture_parses(vectors):
    assert os.path.getsize(PATH) < 200_000
    assert len(vectors) == 3 + 8 * len(LENGTHS) + 1
    assert [len(v.msg) for v in vectors[:3]] == [0, 1, 2]  # RFC 8032 7.1 tests 1-3
    seeds = []
    for v in vectors[3:-1]:
        if v.seed not in seeds:
            seeds.append(v.seed)
    assert len(seeds) == 8
    for s in seeds:
        assert [len(v.msg) for v in vectors[3:-1] if v.seed == s] == LENGTHS
    assert len(vectors[-1].msg) == 4096
    assert vectors[0].sig.hex().startswith("e5564300c360ac72")


def test_every_record_equals_the_oracle_signature(vectors):
    for i, v in enumerate(vectors):
        assert ed25519_ref.sign(v.seed, v.msg) == v.sig, i


def test_every_public_key_equals_the_oracle(vectors):
    for seed in sorted({v.seed for v in vectors}):
        pks = {v.pk for v in vectors if v.seed == seed}
        assert pks == {ed25519_ref.public_key(seed)}


def test_header_declares_the_signing_entries():
    src = open(os.path.join(ROOT, "include", "cbft_hipcrypto.h")).read()
    declared = set(re.findall(r"\b(cbft_[a-z0-9_]+)\s*\(", src))
    for s in SIGN_SYMBOLS:
        assert s in declared, s
        assert s in {n for n, _, _ in cb.ABI}, s


def test_library_exports_the_signing_entries():
    assert os.path.exists(cb.LIB_PATH), "libcbft_hipcrypto.so not built"
    lib = cb.load_library()
    for s in SIGN_SYMBOLS:
        assert hasattr(lib, s), s
