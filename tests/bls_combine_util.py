"""Helpers of the batched BLS combination tests: the host shim (tests/cpp/bls_combine_shim.cpp: the lane
code of csrc/bls_combine_batch.h built for the host), certificates whose combined signature the oracle
gives with one scalar multiplication, and the crafted shares."""
import ctypes
import itertools
import os

import numpy as np

import blsgen
import bn254_ref as B

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def shim():
    global _lib
    if _lib is None:
        path = os.path.join(HERE, "cpp", "libbls_combine_shim.so")
        assert os.path.exists(path), "tests/cpp/libbls_combine_shim.so not built (make bls_combine_shim)"
        _lib = ctypes.CDLL(path)
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def shim_lagrange(ids, use=None):
    """-> ({position: lambda}, state list, dup list) of blsc_lagrange_lane over one certificate"""
    k = len(ids)
    a = np.array(ids, dtype=np.uint32)
    u = None if use is None else np.array(use, dtype=np.uint8)
    lam = np.zeros((max(k, 1), 32), dtype=np.uint8)
    state = np.zeros(max(k, 1), dtype=np.uint8)
    dup = np.zeros(max(k, 1), dtype=np.uint8)
    shim().blsc_shim_lagrange(_p(a), _p(u), k, _p(lam), _p(state), _p(dup))
    out = {j: int.from_bytes(lam[j].tobytes(), "big") for j in range(k) if state[j] == 1 and not dup[j]}
    return out, state[:k].tolist(), dup[:k].tolist()


def shim_mul(p33: bytes, k: int) -> bytes:
    out = ctypes.create_string_buffer(33)
    assert shim().blsc_shim_mul(p33, k.to_bytes(32, "big"), out) == 0
    return out.raw


def shim_batch(certs, use=None, multisig=False):
    """The launch sequence restated on the host: (sigs, status) as Context.bls_combine_batch gives them"""
    m = len(certs)
    off = np.zeros(m + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(c) for c in certs])
    flat = np.frombuffer(b"".join(s for c in certs for s in c) or b"\0", dtype=np.uint8)
    u = None if use is None else np.array(use, dtype=np.uint8)
    out = np.zeros((max(m, 1), 33), dtype=np.uint8)
    status = np.zeros(max(m, 1), dtype=np.uint8)
    shim().blsc_shim_batch(_p(flat), int(off[m]), _p(off), m, _p(u), 1 if multisig else 0, _p(out), _p(status))
    return [out[c].tobytes() for c in range(m)], status[:m]


# ------------------------------------------------------------------------------ expected values
def threshold_value(sk: int, msg: bytes) -> bytes:
    """What ANY k shares of a degree-(k - 1) sharing of sk combine to: one oracle scalar multiplication"""
    return B.g1_to_bytes(B.ec_mul(sk, B.g1_map(msg)))


def multisig_value(shares) -> bytes:
    acc = None
    for s in shares:
        acc = B.ec_add(acc, B.parse_share(s)[1], None)
    return B.g1_to_bytes(acc)


def crafted_value(shares, multisig: bool) -> bytes:
    """Shares that need not lie on one polynomial: the oracle's own combination"""
    if multisig:
        return multisig_value(shares)
    return B.g1_to_bytes(B.combine_threshold({B.parse_share(s)[0]: B.parse_share(s)[1] for s in shares}))


def sharing(n: int, k: int, seed: int, msg: bytes, ids=None):
    """(sk, shares of `ids` (default 1 .. n)) of a k-of-n sharing: from the oracle up to 16 shares, from the
    host build of the device code (blsgen.shares) above"""
    sk, sks = B.keygen(n, k, seed)
    ids = list(range(1, n + 1)) if ids is None else list(ids)
    if len(ids) <= 16:
        return sk, [B.sign_share(sks[i], i, msg) for i in ids]
    return sk, blsgen.shares(sks, ids, msg)


class Pool:
    """`worlds` 5-of-7 sharings, each with its own message and all seven shares from the oracle.
    cert(c): five of world c % worlds' seven shares, a different subset from one lap to the next, so the
    certificates of a batch all differ while the oracle does one scalar multiplication per world."""

    N, K = 7, 5

    def __init__(self, worlds: int = 16, seed: int = 0x24A):
        self.worlds = worlds
        self.msg = [b"combine batch %d" % w for w in range(worlds)]
        made = [sharing(self.N, self.K, seed + w, self.msg[w]) for w in range(worlds)]
        self.sk = [sk for sk, _ in made]
        self.shares = [sh for _, sh in made]
        self.want = [threshold_value(self.sk[w], self.msg[w]) for w in range(worlds)]
        self.subsets = list(itertools.combinations(range(self.N), self.K))

    def cert(self, c: int):
        w = c % self.worlds
        sub = self.subsets[(c // self.worlds * 5 + w) % len(self.subsets)]
        return [self.shares[w][j] for j in sub]

    def expected(self, c: int) -> bytes:
        return self.want[c % self.worlds]


def off_curve_x() -> int:
    return next(x for x in range(1, 100) if pow((x ** 3 + 2) % B.P, (B.P - 1) // 2, B.P) != 1)


def with_id(share: bytes, i: int) -> bytes:
    return i.to_bytes(4, "big") + share[4:]


def negated(share: bytes) -> bytes:
    i, s = B.parse_share(share)
    return share[:4] + B.g1_to_bytes(B.ec_neg(s))
