"""Helpers of the Ed25519 signing tests: the golden fixture's reader and host OpenSSL signing."""
import os
import struct
from typing import List, NamedTuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "ed25519_sign_vectors.bin")
MAGIC = b"CBFTEDSIGNV1\0\0\0\0"


class SignVector(NamedTuple):
    seed: bytes
    pk: bytes
    sig: bytes
    msg: bytes


def load_sign_vectors(path: str = PATH) -> List[SignVector]:
    raw = open(path, "rb").read()
    assert raw[:16] == MAGIC, "not an Ed25519 signing fixture"
    (count,) = struct.unpack_from("<I", raw, 16)
    pos, out = 20, []
    for _ in range(count):
        (mlen,) = struct.unpack_from("<I", raw, pos)
        pos += 4
        seed, pk, sig = raw[pos:pos + 32], raw[pos + 32:pos + 64], raw[pos + 64:pos + 128]
        pos += 128
        out.append(SignVector(seed, pk, sig, raw[pos:pos + mlen]))
        pos += mlen
    assert pos == len(raw), "trailing bytes"
    return out


class Hip:
    """Device buffers and streams from the HIP runtime libcbft_hipcrypto itself links (as
    tests/test_ed25519_gpu.py: a second runtime in the process would see no GPU)."""

    def __init__(self):
        import ctypes

        import cbft_hipcrypto as cb

        cb.load_library()
        self.ct = ctypes
        self.lib = ctypes.CDLL("libamdhip64.so.7")
        self.bufs, self.streams = [], []

    def _ok(self, rc, what):
        assert rc == 0, f"{what}: hipError {rc}"

    def to_dev(self, a: np.ndarray) -> int:
        ct = self.ct
        p = ct.c_void_p()
        self._ok(self.lib.hipMalloc(ct.byref(p), ct.c_size_t(max(a.nbytes, 1))), "hipMalloc")
        self.bufs.append(p.value)
        a = np.ascontiguousarray(a)
        self._ok(self.lib.hipMemcpy(p, a.ctypes.data_as(ct.c_void_p), ct.c_size_t(a.nbytes), 1), "hipMemcpy")
        return p.value

    def from_dev(self, ptr: int, nbytes: int) -> np.ndarray:
        ct = self.ct
        out = np.zeros(nbytes, dtype=np.uint8)
        self._ok(self.lib.hipMemcpy(out.ctypes.data_as(ct.c_void_p), ct.c_void_p(ptr), ct.c_size_t(nbytes), 2),
                 "hipMemcpy")
        return out

    def stream(self) -> int:
        s = self.ct.c_void_p()
        self._ok(self.lib.hipStreamCreate(self.ct.byref(s)), "hipStreamCreate")
        self.streams.append(s.value)
        return s.value

    def sync(self):
        self._ok(self.lib.hipDeviceSynchronize(), "hipDeviceSynchronize")

    def close(self):
        self.sync()
        for s in self.streams:
            self.lib.hipStreamDestroy(self.ct.c_void_p(s))
        for b in self.bufs:
            self.lib.hipFree(self.ct.c_void_p(b))


def openssl_sign_many(seeds: np.ndarray, key_idx: np.ndarray, blob: np.ndarray, off: np.ndarray, lens: np.ndarray,
                      threads: int = 8) -> np.ndarray:
    """(n, 64) uint8: host OpenSSL EVP_DigestSign of message i under seeds[key_idx[i]]."""
    import ctypes

    import workload

    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    seeds = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(-1, 32)
    key_idx = np.ascontiguousarray(key_idx, dtype=np.uint32)
    n = int(lens.shape[0])
    sig = np.zeros((max(n, 1), 64), dtype=np.uint8)
    rc = workload.cpu_lib().cbft_cpu_sign_many(p(seeds), seeds.shape[0], p(key_idx), p(blob), p(off), p(lens), n,
                                               p(sig), threads)
    assert rc == 0, f"cbft_cpu_sign_many: {rc}"
    return sig[:n]
