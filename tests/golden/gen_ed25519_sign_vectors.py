#!/usr/bin/env python3
"""Generate tests/golden/ed25519_sign_vectors.bin — golden Ed25519 signing vectors.

Ground truth: OpenSSL 3.0.2 libcrypto (EVP_PKEY_new_raw_private_key(ED25519) + EVP_DigestSign), the
library the reference signs with.  Ed25519 signatures are deterministic (RFC 8032 §5.1.6), so the
GPU signer must reproduce every byte.  The generator asserts that every record also equals the
pure-Python restatement oracle/ed25519_ref.py (sign and public_key).

Contents: RFC 8032 §7.1 tests 1-3; 8 seeds x the message lengths whose SHA-512 padding falls on a
block edge of either hash (47/48, 175/176: R || A || M; 79/80, 207/208: prefix || M) and their
neighbours; one 4,096-byte message.

Record format (little-endian), after the 16-byte header b"CBFTEDSIGNV1\\0\\0\\0\\0" + u32 count:
    u32 msg_len | seed[32] | pk[32] | sig[64] | msg[msg_len]
Run:  python3 tests/golden/gen_ed25519_sign_vectors.py   (needs libcrypto.so.3)
"""
from __future__ import annotations

import ctypes
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import ed25519_ref as E  # noqa: E402
from gen_ed25519_vectors import RFC8032  # noqa: E402

MAGIC = b"CBFTEDSIGNV1\0\0\0\0"
LENGTHS = [0, 1, 31, 32, 47, 48, 63, 64, 79, 80, 111, 112, 127, 128, 175, 176, 207, 208, 239, 240, 256, 1023]
NSEEDS = 8


class OpenSSLSigner:
    NID_ED25519 = 1087

    def __init__(self):
        self.lib = ctypes.CDLL("libcrypto.so.3")
        L = self.lib
        L.EVP_PKEY_new_raw_private_key.restype = ctypes.c_void_p
        L.EVP_PKEY_new_raw_private_key.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.EVP_PKEY_get_raw_public_key.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t)]
        L.EVP_MD_CTX_new.restype = ctypes.c_void_p
        L.EVP_MD_CTX_free.argtypes = [ctypes.c_void_p]
        L.EVP_PKEY_free.argtypes = [ctypes.c_void_p]
        L.EVP_DigestSignInit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]
        L.EVP_DigestSign.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t),
                                     ctypes.c_char_p, ctypes.c_size_t]

    def sign(self, seed: bytes, msg: bytes):
        """(public key, signature) of msg under the RFC 8032 private key `seed`."""
        L = self.lib
        key = L.EVP_PKEY_new_raw_private_key(self.NID_ED25519, None, seed, 32)
        assert key, "raw private key rejected"
        ctx = L.EVP_MD_CTX_new()
        try:
            pk = ctypes.create_string_buffer(32)
            n = ctypes.c_size_t(32)
            assert L.EVP_PKEY_get_raw_public_key(key, pk, ctypes.byref(n)) == 1 and n.value == 32
            assert L.EVP_DigestSignInit(ctx, None, None, None, key) == 1
            sig = ctypes.create_string_buffer(64)
            n = ctypes.c_size_t(64)
            assert L.EVP_DigestSign(ctx, sig, ctypes.byref(n), msg, len(msg)) == 1 and n.value == 64
            return pk.raw, sig.raw
        finally:
            L.EVP_MD_CTX_free(ctx)
            L.EVP_PKEY_free(key)


def main():
    rng = random.Random(0x51C9ED)
    ossl = OpenSSLSigner()
    recs = []

    def add(seed: bytes, msg: bytes):
        pk, sig = ossl.sign(seed, msg)
        assert pk == E.public_key(seed), "OpenSSL vs ed25519_ref public key"
        assert sig == E.sign(seed, msg), "OpenSSL vs ed25519_ref signature"
        recs.append((seed, pk, sig, msg))
        return pk, sig

    for sk, pk, msg, sig in RFC8032:
        got_pk, got_sig = add(bytes.fromhex(sk), bytes.fromhex(msg))
        assert got_pk.hex() == pk and got_sig.hex() == sig, "RFC 8032 7.1"

    seeds = [rng.randbytes(32) for _ in range(NSEEDS)]
    for seed in seeds:
        for m in LENGTHS:
            add(seed, rng.randbytes(m))
    add(seeds[0], rng.randbytes(4096))

    out = os.path.join(HERE, "ed25519_sign_vectors.bin")
    with open(out, "wb") as f:
        f.write(MAGIC + struct.pack("<I", len(recs)))
        for seed, pk, sig, msg in recs:
            f.write(struct.pack("<I", len(msg)) + seed + pk + sig + msg)
    print(f"wrote {len(recs)} signing vectors, {os.path.getsize(out)} bytes -> {out}")


if __name__ == "__main__":
    main()
