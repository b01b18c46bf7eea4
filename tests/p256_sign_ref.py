"""Deterministic ECDSA P-256 (secp256r1) / SHA-256 signing (RFC 6979 nonces, r || s, no low-s rule)
restated on hmac, hashlib and Python integers: the byte reference of cbft_ecdsa_load_signers_curve
(CBFT_CURVE_P256) in include/cbft_hipcrypto.h.  The nonce generator is tests/ecdsa_sign_ref.py's with
P-256's order, the curve arithmetic is tests/p256_ref.py's; RFC 6979 A.2.5 pins both
(tests/golden/gen_ecdsa_p256_sign_vectors.py)."""
import hashlib

import ecdsa_sign_ref as sref
import p256_ref as ref

N = ref.N


def nonce(x: int, h1: bytes, with_rejections: bool = False):
    """The first candidate in [1, n - 1]."""
    return sref.nonce(x, h1, N, with_rejections)


def sign_with_k(x: int, e: int, k: int):
    """(r, s) for the digest integer e (already reduced or not) and the nonce k; None when r or s is 0."""
    R = ref.mul(k, ref.G)
    r = R[0] % N
    s = pow(k, -1, N) * (e + r * x) % N
    return (r, s) if r and s else None


def sign_digest(x: int, h1: bytes, e=None):
    """(k, r, s): r = 0 or s = 0 sends the generator to its next candidate like an out-of-range one.
    e: the integer that enters s, h1 mod n unless a test of the retry path gives another."""
    assert 1 <= x < N
    if e is None:
        e = int.from_bytes(h1, "big") % N
    d = sref.Drbg(x, h1, N)
    while True:
        k = d.candidate()
        if 1 <= k < N:
            rs = sign_with_k(x, e, k)
            if rs:
                return (k,) + rs
        d.reject()


def sign(x: int, msg: bytes) -> bytes:
    _, r, s = sign_digest(x, hashlib.sha256(msg).digest())
    return ref.sig_bytes(r, s)


def public_key(x: int) -> bytes:
    return ref.pub_bytes(ref.mul(x, ref.G))
