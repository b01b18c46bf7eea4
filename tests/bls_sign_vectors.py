"""Helpers of the batched BLS signing tests: the golden fixture's reader / writer and the host shim
(tests/cpp/bls_sign_shim.cpp: the lane routine of csrc/bls_sign_batch.h built for the host)."""
import ctypes
import json
import os
from typing import List, NamedTuple, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "bls_sign_vectors.json")
FORMAT = "cbft-bls-sign-vectors-1"


class BlsSignVector(NamedTuple):
    signer: int   # index into the fixture's signers
    msg: bytes
    inc: int      # increments the hash to G1 needs
    share: bytes  # 37 bytes: be32(id) || compressed sigma


def dump_fixture(path: str, signers: List[Tuple[int, int]], vectors: List[BlsSignVector]) -> None:
    doc = {"format": FORMAT,
           "signers": [{"sk": f"{sk:064x}", "id": sid} for sk, sid in signers],
           "vectors": [{"signer": v.signer, "msg": v.msg.hex(), "inc": v.inc, "share": v.share.hex()}
                       for v in vectors]}
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")


def load_fixture(path: str = PATH):
    """-> (signers: [(sk, id)], vectors: [BlsSignVector])"""
    doc = json.load(open(path))
    assert doc["format"] == FORMAT, "not a BLS signing fixture"
    signers = [(int(s["sk"], 16), int(s["id"])) for s in doc["signers"]]
    vectors = [BlsSignVector(int(v["signer"]), bytes.fromhex(v["msg"]), int(v["inc"]), bytes.fromhex(v["share"]))
               for v in doc["vectors"]]
    return signers, vectors


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


_lib = None


def sign_shim():
    global _lib
    if _lib is None:
        path = os.path.join(HERE, "cpp", "libbls_sign_shim.so")
        assert os.path.exists(path), "tests/cpp/libbls_sign_shim.so not built (make bls_sign_shim)"
        _lib = ctypes.CDLL(path)
        _lib.bls_sign_shim_addsub_random.restype = ctypes.c_long
        _lib.bls_sign_shim_addsub_ties.restype = ctypes.c_long
    return _lib


def pack(msgs):
    lens = np.array([len(m) for m in msgs], dtype=np.uint32)
    off = np.zeros(len(msgs), dtype=np.uint64)
    if len(msgs) > 1:
        np.cumsum(lens[:-1].astype(np.uint64), out=off[1:])
    blob = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()
    return blob, off, lens


def lane_sign_many(signers, signer_idx, msgs, threads: int = 16, window: int = 0):
    """The host build of the lane routine (window 3 or 4; 0 = the one the product runs): (n, 37) uint8
    shares and the increments each hash took."""
    n = len(msgs)
    sks = np.frombuffer(b"".join(sk.to_bytes(32, "big") for sk, _ in signers), dtype=np.uint8).copy()
    ids = np.array([sid for _, sid in signers], dtype=np.uint32)
    idx = np.ascontiguousarray(np.asarray(signer_idx, dtype=np.uint32))
    blob, off, lens = pack(msgs)
    out = np.zeros((max(n, 1), 37), dtype=np.uint8)
    incs = np.zeros(max(n, 1), dtype=np.int32)
    sign_shim().bls_sign_shim_shares_mt(window, _p(sks), _p(ids), _p(idx), _p(blob), _p(off), _p(lens), n, _p(out), _p(incs),
                                        threads)
    return out[:n], incs[:n]


def row_shim_sign_many(signers, signer_idx, msgs):
    """tests/cpp/bn254_shim.cpp shim_sign_share: plain double-and-add, independent of the lane routine."""
    lib = ctypes.CDLL(os.path.join(HERE, "cpp", "libbn254_shim.so"))
    out = np.zeros((max(len(msgs), 1), 37), dtype=np.uint8)
    buf = ctypes.create_string_buffer(37)
    for i, (s, m) in enumerate(zip(signer_idx, msgs)):
        sk, sid = signers[s]
        lib.shim_sign_share(sk.to_bytes(32, "big"), sid, m, len(m), buf)
        out[i] = np.frombuffer(buf.raw, dtype=np.uint8)
    return out[:len(msgs)]
