"""Deterministic ECDSA secp256k1 / SHA-256 signing (RFC 6979 nonces, r || s, no low-s rule) restated
on hmac, hashlib and Python integers: the byte reference of include/cbft_hipcrypto.h's ECDSA signing
section.  The curve arithmetic is tests/ecdsa_ref.py's.  The nonce function takes the group order as
an argument (any order of 256 bits: qlen == hlen == 256), so the RFC's own P-256 vectors pin it."""
import hashlib
import hmac

import ecdsa_ref as ref

N = ref.N


def bits2octets(h1: bytes, q: int) -> bytes:
    z = int.from_bytes(h1, "big")
    return (z - q if z >= q else z).to_bytes(32, "big")


class Drbg:
    """RFC 6979 section 3.2, steps b to h, for a 256-bit order q; candidates one by one."""

    def __init__(self, x: int, h1: bytes, q: int):
        assert q.bit_length() == 256 and len(h1) == 32
        self.q = q
        seed = x.to_bytes(32, "big") + bits2octets(h1, q)
        self.V, self.K = b"\x01" * 32, b"\x00" * 32
        self.K = self._mac(self.V + b"\x00" + seed)
        self.V = self._mac(self.V)
        self.K = self._mac(self.V + b"\x01" + seed)
        self.V = self._mac(self.V)
        self.rejected = 0

    def _mac(self, data: bytes) -> bytes:
        return hmac.new(self.K, data, hashlib.sha256).digest()

    def candidate(self) -> int:
        """The next candidate as an integer (any 256-bit value: the caller range-tests it)."""
        self.V = self._mac(self.V)
        return int.from_bytes(self.V, "big")

    def reject(self):
        self.K = self._mac(self.V + b"\x00")
        self.V = self._mac(self.V)
        self.rejected += 1


def nonce(x: int, h1: bytes, q: int = N, with_rejections: bool = False):
    """The first candidate in [1, q - 1]."""
    d = Drbg(x, h1, q)
    while True:
        k = d.candidate()
        if 1 <= k < q:
            return (k, d.rejected) if with_rejections else k
        d.reject()


def sign_with_k(x: int, e: int, k: int):
    """(r, s) for the digest integer e (already reduced or not) and the nonce k; None when r or s is 0."""
    R = ref.mul(k, ref.G)
    r = R[0] % N
    s = pow(k, -1, N) * (e + r * x) % N
    return (r, s) if r and s else None


def sign_digest(x: int, h1: bytes):
    """(k, r, s): r = 0 or s = 0 sends the generator to its next candidate like an out-of-range one."""
    assert 1 <= x < N
    e = int.from_bytes(h1, "big") % N
    d = Drbg(x, h1, N)
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
