#!/usr/bin/env python3
"""Generate tests/golden/rsa_sign_vectors.json — golden RSA-2048 PKCS#1 v1.5 / SHA-256 signatures.

Ground truth: OpenSSL 3.0.2 libcrypto (d2i_AutoPrivateKey of a PKCS#1 RSAPrivateKey built from the
key's integers, then EVP_DigestSign with SHA-256).  PKCS#1 v1.5 signatures are deterministic, so
the GPU signer must reproduce every byte.  The generator asserts that every signature also equals
the restatement oracle/rsa_ref.py:sign of the reference's Crypto++ signer.

Contents: the eight keys of tests/golden/rsa_test_keys.json (e = 3, 17, 65537, 0xC0000001; both
prime orders) x the message lengths around the SHA-256 padding edges (55/56, 63/64, 119/120) and
0, 1, 32, 128, 256; one 4,096-byte message.

Format: {"vectors": [{"key": index into rsa_test_keys.json, "msg": hex, "sig": hex}, ...]}
Run:  python3 tests/golden/gen_rsa_sign_vectors.py   (needs libcrypto.so.3)
"""
from __future__ import annotations

import ctypes
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))
import rsa_ref  # noqa: E402
import rsagen  # noqa: E402

LENGTHS = [0, 1, 32, 55, 56, 63, 64, 119, 120, 128, 256]


def _der_len(n: int) -> bytes:
    if n < 0x80:
        return bytes([n])
    b = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([0x80 | len(b)]) + b


def _der_int(v: int) -> bytes:
    b = v.to_bytes(v.bit_length() // 8 + 1, "big")  # a leading 0x00 keeps it non-negative
    return b"\x02" + _der_len(len(b)) + b


def pkcs1_der(key) -> bytes:
    """RSAPrivateKey ::= SEQUENCE { 0, n, e, d, p, q, d mod (p-1), d mod (q-1), q^-1 mod p }"""
    p, q, d = key["p"], key["q"], key["d"]
    body = b"".join(_der_int(v) for v in (0, key["n"], key["e"], d, p, q, d % (p - 1), d % (q - 1), pow(q, -1, p)))
    return b"\x30" + _der_len(len(body)) + body


class OpenSSLRsaSigner:
    def __init__(self):
        self.lib = ctypes.CDLL("libcrypto.so.3")
        L = self.lib
        L.d2i_AutoPrivateKey.restype = ctypes.c_void_p
        L.d2i_AutoPrivateKey.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_long]
        L.EVP_MD_CTX_new.restype = ctypes.c_void_p
        L.EVP_MD_CTX_free.argtypes = [ctypes.c_void_p]
        L.EVP_PKEY_free.argtypes = [ctypes.c_void_p]
        L.EVP_sha256.restype = ctypes.c_void_p
        L.EVP_DigestSignInit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]
        L.EVP_DigestSign.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t),
                                     ctypes.c_char_p, ctypes.c_size_t]

    def sign(self, key, msg: bytes) -> bytes:
        L = self.lib
        der = pkcs1_der(key)
        ptr = ctypes.c_char_p(der)
        pkey = L.d2i_AutoPrivateKey(None, ctypes.byref(ptr), len(der))
        assert pkey, "PKCS#1 key rejected"
        ctx = L.EVP_MD_CTX_new()
        try:
            assert L.EVP_DigestSignInit(ctx, None, L.EVP_sha256(), None, pkey) == 1
            sig = ctypes.create_string_buffer(256)
            n = ctypes.c_size_t(256)
            assert L.EVP_DigestSign(ctx, sig, ctypes.byref(n), msg, len(msg)) == 1 and n.value == 256
            return sig.raw
        finally:
            L.EVP_MD_CTX_free(ctx)
            L.EVP_PKEY_free(pkey)


def main():
    rng = random.Random(0x25A519)
    keys = rsagen.load_keys()
    ossl = OpenSSLRsaSigner()
    vecs = []

    def add(ki: int, msg: bytes):
        sig = ossl.sign(keys[ki], msg)
        assert sig == rsa_ref.sign(keys[ki]["n"], keys[ki]["d"], msg), "OpenSSL vs rsa_ref.sign"
        vecs.append({"key": ki, "msg": msg.hex(), "sig": sig.hex()})

    for ki in range(len(keys)):
        for m in LENGTHS:
            add(ki, rng.randbytes(m))
    add(0, rng.randbytes(4096))
    out = os.path.join(HERE, "rsa_sign_vectors.json")
    with open(out, "w") as f:
        json.dump({"note": "OpenSSL 3.0.2 EVP_DigestSign (RSA, SHA-256) over rsa_test_keys.json "
                           "(tests/golden/gen_rsa_sign_vectors.py)", "vectors": vecs}, f, indent=0)
    print(f"wrote {len(vecs)} signing vectors, {os.path.getsize(out)} bytes -> {out}")


if __name__ == "__main__":
    main()
