#!/usr/bin/env python3
"""Generates tests/golden/ecdsa_p256_sign_vectors.json: deterministic ECDSA P-256 / SHA-256 signatures
(RFC 6979 nonces, r || s, no low-s rule) from tests/p256_sign_ref.py.  Asserts RFC 6979 A.2.5 in full
(the key's public point, and k, r, s for "sample" and "test" with SHA-256) and that OpenSSL's
ECDSA_do_verify on prime256v1 accepts every signature.  Deterministic.

    python3 tests/golden/gen_ecdsa_p256_sign_vectors.py

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
import p256_ref as ref  # noqa: E402
import p256_sign_ref as sref  # noqa: E402
from gen_ecdsa_p256_vectors import openssl_verdict  # noqa: E402

N = ref.N
LENGTHS = (0, 1, 31, 32, 55, 56, 63, 64, 65, 119, 120, 256, 4096)
A25_X = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
A25 = (
    (b"sample", 0xA6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60,
     0xEFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716,
     0xF7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8),
    (b"test", 0xD16B6AE827F17175E040871A1C7EC3500192C4C92677336EC2537ACAEE0008E0,
     0xF1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367,
     0x019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083),
)


def edge_keys():
    keys = [1, 2, 3, N - 1, N - 2, 1 << 128, 1 << 255]
    for j in (1, 2, 31, 32, 63):
        keys += [16**j, 16**j - 1]
    keys.append(int("8" * 64, 16) % N)
    return keys


def check_anchors():
    assert ref.mul(A25_X, ref.G) == (0x60FED4BA255A9D31C961EB74C6356D68C049B8923B61FA6CE669622E60F29FB6,
                                     0x7903FE1008B8BC99A41AE9E95628BC64F2F1B20C2D7E9F5177A3C294D4462299)
    for msg, k, r, s in A25:
        assert sref.sign_digest(A25_X, hashlib.sha256(msg).digest()) == (k, r, s), msg


def main():
    check_anchors()
    rng = random.Random(0xEC5256)
    cases = []
    for i, x in enumerate(edge_keys()):
        for ln in (LENGTHS[i % 12], LENGTHS[(i + 5) % 12]):
            cases.append((x, rng.randbytes(ln)))
    for _ in range(12):
        x = rng.randrange(1, N)
        for ln in LENGTHS[:12]:
            cases.append((x, rng.randbytes(ln)))
    for x in (N - 1, rng.randrange(1, N)):  # two, not three: the file stays below ecdsa_sign_vectors.json's size
        cases.append((x, rng.randbytes(4096)))
    for msg, _, _, _ in A25:
        cases.append((A25_X, msg))
    vectors = []
    for x, msg in cases:
        k, r, s = sref.sign_digest(x, hashlib.sha256(msg).digest())
        sig = ref.sig_bytes(r, s)
        assert sig == sref.sign(x, msg)
        assert openssl_verdict(sref.public_key(x), sig, msg) == 1, (hex(x), msg.hex())
        vectors.append({"x": f"{x:064x}", "msg": msg.hex(), "k": f"{k:064x}", "sig": sig.hex()})
    path = os.path.join(HERE, "ecdsa_p256_sign_vectors.json")
    with open(path, "w") as f:
        json.dump({"vectors": vectors}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(vectors)} vectors, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
