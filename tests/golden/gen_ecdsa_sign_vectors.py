#!/usr/bin/env python3
"""Generates tests/golden/ecdsa_sign_vectors.json: deterministic ECDSA secp256k1 / SHA-256 signatures
(RFC 6979 nonces, r || s, no low-s rule) from tests/ecdsa_sign_ref.py.  Asserts the RFC 6979 A.2.5
nonces (P-256 order: the derivation does not depend on the curve), the secp256k1 vector for x = 1 /
"Satoshi Nakamoto" (its published form carries n - s: it applies the low-s rule, we do not), and that
OpenSSL's ECDSA_do_verify accepts every signature.  Deterministic.

    python3 tests/golden/gen_ecdsa_sign_vectors.py

File: {"vectors": [{"x", "msg", "k", "sig"}]}, all hex; sig = r || s.
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ecdsa_ref as ref  # noqa: E402
import ecdsa_sign_ref as sref  # noqa: E402
from gen_ecdsa_vectors import openssl_verdict  # noqa: E402

N = ref.N
P256_N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
LENGTHS = (0, 1, 31, 32, 55, 56, 63, 64, 65, 119, 120, 256, 4096)


def edge_keys():
    keys = [1, 2, 3, N - 1, N - 2, 1 << 128, 1 << 255]
    for j in (1, 2, 31, 32, 63):
        keys += [16**j, 16**j - 1]
    keys.append(int("8" * 64, 16) % N)
    return keys


def check_anchors():
    x = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
    for msg, k in ((b"sample", 0xA6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60),
                   (b"test", 0xD16B6AE827F17175E040871A1C7EC3500192C4C92677336EC2537ACAEE0008E0)):
        assert sref.nonce(x, hashlib.sha256(msg).digest(), P256_N) == k, msg
    k, r, s = sref.sign_digest(1, hashlib.sha256(b"Satoshi Nakamoto").digest())
    assert k == 0x8F8A276C19F4149656B280621E358CCE24F5F52542772691EE69063B74F15D15
    assert r == 0x934B1EA10A4B3C1757E2B0C017D0B6143CE3C9A7E6A4A49860D7A6AB210EE3D8
    assert s == 0xDBBD3162D46E9F9BEF7FEB87C16DC13B4F6568A87F4E83F728E2443BA586675C


def main():
    check_anchors()
    rng = random.Random(0xEC5161)
    cases = []
    for i, x in enumerate(edge_keys()):
        for ln in (LENGTHS[i % 12], LENGTHS[(i + 5) % 12]):
            cases.append((x, rng.randbytes(ln)))
    for _ in range(12):
        x = rng.randrange(1, N)
        for ln in LENGTHS[:12]:
            cases.append((x, rng.randbytes(ln)))
    for x in (1, N - 1, rng.randrange(1, N)):
        cases.append((x, rng.randbytes(4096)))
    cases.append((1, b"Satoshi Nakamoto"))
    vectors = []
    for x, msg in cases:
        k, r, s = sref.sign_digest(x, hashlib.sha256(msg).digest())
        sig = ref.sig_bytes(r, s)
        assert sig == sref.sign(x, msg)
        assert openssl_verdict(sref.public_key(x), sig, msg) == 1, (hex(x), msg.hex())
        vectors.append({"x": f"{x:064x}", "msg": msg.hex(), "k": f"{k:064x}", "sig": sig.hex()})
    path = os.path.join(HERE, "ecdsa_sign_vectors.json")
    with open(path, "w") as f:
        json.dump({"vectors": vectors}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(vectors)} vectors, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
