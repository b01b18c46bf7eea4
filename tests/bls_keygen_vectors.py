"""Helpers of the batched BLS key derivation tests: the golden fixture's reader / writer, the host shim
(tests/cpp/bls_keygen_shim.cpp: the lane routines of csrc/bls_keygen_batch.h built for the host) and the
plain double-and-add of tests/cpp/bn254_shim.cpp."""
import ctypes
import json
import os
from typing import List, NamedTuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "bls_keygen_vectors.json")
FORMAT = "cbft-bls-keygen-vectors-1"

R = 0x2523648240000001BA344D8000000007FF9F800000000010A10000000000000D
ZERO65 = bytes(65)


class BlsKeygenVector(NamedTuple):
    cls: str   # the edge class the scalar stands for
    sk: int    # any value below 2^256
    vk: bytes  # 65 bytes: (sk mod r) * g2 compressed, zeros where sk = 0 mod r
    ok: int


def dump_fixture(path: str, vectors: List[BlsKeygenVector]) -> None:
    doc = {"format": FORMAT,
           "vectors": [{"class": v.cls, "sk": f"{v.sk:064x}", "vk": v.vk.hex(), "ok": v.ok} for v in vectors]}
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")


def load_fixture(path: str = PATH) -> List[BlsKeygenVector]:
    doc = json.load(open(path))
    assert doc["format"] == FORMAT, "not a BLS keygen fixture"
    return [BlsKeygenVector(v["class"], int(v["sk"], 16), bytes.fromhex(v["vk"]), int(v["ok"])) for v in doc["vectors"]]


def recoded_nibbles(sk: int):
    """The 64 radix-16 digits nib_j of u = (k' + 2^256 - 1) / 2 that the comb reads for sk (not 0 mod r):
    digit d_j = 2 nib_j - 15, k' = sk mod r made odd by r - k."""
    k = sk % R
    assert k
    if k % 2 == 0:
        k = R - k
    u = (k + 2**256 - 1) // 2
    return [(u >> (4 * j)) & 15 for j in range(64)]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


_lib = None
_bn = None


def keygen_shim():
    global _lib
    if _lib is None:
        path = os.path.join(HERE, "cpp", "libbls_keygen_shim.so")
        assert os.path.exists(path), "tests/cpp/libbls_keygen_shim.so not built (make bls_keygen_shim)"
        _lib = ctypes.CDLL(path)
        _lib.bls_keygen_shim_fp2_random.restype = ctypes.c_long
        _lib.bls_keygen_shim_fp2_ties.restype = ctypes.c_long
    return _lib


def bn_shim():
    global _bn
    if _bn is None:
        path = os.path.join(HERE, "cpp", "libbn254_shim.so")
        assert os.path.exists(path), "tests/cpp/libbn254_shim.so not built (make shim)"
        _bn = ctypes.CDLL(path)
    return _bn


def sk_bytes(sks) -> np.ndarray:
    return np.frombuffer(b"".join(int(x).to_bytes(32, "big") for x in sks) or bytes(32), dtype=np.uint8).copy()


def lane_keys(sks, threads: int = 16):
    """The host build of bls_keygen_lane over any scalars below 2^256: ([65-byte keys], ok bytes)."""
    n = len(sks)
    out = np.zeros((max(n, 1), 65), dtype=np.uint8)
    ok = np.full(max(n, 1), 2, dtype=np.uint8)
    keygen_shim().bls_keygen_shim_keys_mt(_p(sk_bytes(sks)), n, _p(out), _p(ok), threads)
    return [out[i].tobytes() for i in range(n)], ok[:n]


def plain_keys(sks, threads: int = 16):
    """(sk mod r) * g2 by the plain double-and-add of the branching host code (shim_g2_mul_gen_mt); zeros
    where the scalar is 0 mod r."""
    n = len(sks)
    red = [int(x) % R for x in sks]
    out = np.zeros((max(n, 1), 65), dtype=np.uint8)
    bn_shim().shim_g2_mul_gen_mt(_p(sk_bytes(red)), n, _p(out), threads)
    return [out[i].tobytes() if red[i] else ZERO65 for i in range(n)]


def lane_reduce(x: int) -> int:
    src = np.frombuffer(int(x).to_bytes(32, "big"), dtype=np.uint8).copy()
    dst = np.zeros(32, dtype=np.uint8)
    keygen_shim().bls_keygen_shim_reduce(_p(src), _p(dst))
    return int.from_bytes(dst.tobytes(), "big")


def lane_deal(coeffs, n: int):
    """The dealing as the kernels run it: [c_0 mod r, f(1), .., f(n)]."""
    out = np.zeros((n + 1, 32), dtype=np.uint8)
    keygen_shim().bls_keygen_shim_deal(_p(sk_bytes(coeffs)), len(coeffs), n, _p(out))
    return [int.from_bytes(out[i].tobytes(), "big") for i in range(n + 1)]


def horner(coeffs, x: int) -> int:
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc
