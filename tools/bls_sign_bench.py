#!/usr/bin/env python3
"""Measures batched BLS share signing and writes profiles/bls_sign.json.

One run, one GPU.  Every share of every timed leg is first compared with the host shim's plain
double-and-add (tests/cpp/bn254_shim.cpp shim_sign_share) and a sample with the Python oracle; a
mismatch aborts the run.  Legs:

  batch       cbft_bls_sign_fixed_device (device-resident) and cbft_bls_sign_batch (host arrays in,
              host arrays out) at 65,536 x 32 B and 4,096 x 32 B, one signer
  lone        a loop of cbft_bls_sign over 256 of the same messages (the rate before this entry existed)
  host        the lane routine built for the host on 16 threads ("port, not RELIC")
  crossover   one batch call against n lone calls, n = 1 .. 64 (sets CBFT_BLS_SIGN_BATCH_MIN_DEFAULT)
  kernels     hash and multiplication kernel times of the kept geometry and of the rejected variants
              (plain hash loop; window 4 with the table in LDS or in global scratch) from
              tests/hip/libbls_sign_selftest.so, with the hash kernel's rounds per wave

    python tools/bls_sign_bench.py [--out profiles/bls_sign.json] [--quick]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("concord-bft_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import blsgen  # noqa: E402
import bn254_ref as B  # noqa: E402
import cbft_hipcrypto as cb  # noqa: E402
from bls_sign_vectors import lane_sign_many, sign_shim  # noqa: E402
from sign_vectors import Hip  # noqa: E402

# registers / LDS / scratch per kernel as the compiler reports them for gfx950
# (hipcc -Rpass-analysis=kernel-resource-usage on csrc/bls_sign_batch.hip and tests/hip/bls_sign_selftest.hip)
RESOURCES = {
    "bls_sign_hash_kernel<steal>": {"vgpr": 248, "agpr": 32, "scratch_bytes": 768, "lds_bytes": 4, "waves_per_simd": 1},
    "bls_sign_hash_kernel<plain>": {"vgpr": 248, "agpr": 32, "scratch_bytes": 768, "lds_bytes": 4, "waves_per_simd": 1},
    "bls_sign_mul_kernel<window 3, LDS table> (kept)": {"vgpr": 224, "agpr": 0, "scratch_bytes": 832,
                                                         "lds_bytes": 27648, "waves_per_simd": 2},
    "bls_sign_mul_kernel<window 4, LDS table>": {"vgpr": 224, "agpr": 0, "scratch_bytes": 832, "lds_bytes": 55296,
                                                  "waves_per_simd": 1},
    "bls_sign_mul_kernel<window 4, global table>": {"vgpr": 256, "agpr": 256, "scratch_bytes": 1104, "lds_bytes": 0,
                                                     "waves_per_simd": 1},
}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def shim_shares(sk, sid, msgs):
    def one(m):
        out = ctypes.create_string_buffer(37)
        blsgen.shim().shim_sign_share(blsgen.be32(sk), sid, m, len(m), out)
        return out.raw
    with ThreadPoolExecutor(16) as ex:
        rows = list(ex.map(one, msgs, chunksize=64))
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(msgs), 37)


def check(name, got, exp, sk, sid, msgs, rng):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    if bad.size:
        raise SystemExit(f"{name}: {bad.size} of {len(msgs)} shares differ from the shim, first {bad[:8]}")
    for i in rng.sample(range(len(msgs)), min(len(msgs), 8)):
        if got[i].tobytes() != B.sign_share(sk, sid, msgs[i]):
            raise SystemExit(f"{name}: share {i} differs from the oracle")


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return ts


def rate_entry(n, ts):
    med = statistics.median(ts)
    return {"n": n, "reps": len(ts), "ms_median": round(1e3 * med, 4), "ms_min": round(1e3 * min(ts), 4),
            "shares_per_s_median": round(n / med, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bls_sign.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal, not a measurement)")
    a = ap.parse_args()
    sizes = [1024, 256] if a.quick else [65536, 4096]
    reps = 3 if a.quick else 7
    rng = random.Random(0xB15)
    sk, sid = rng.randrange(1, B.R), 9
    nmax = max(sizes)
    msgs = [rng.randbytes(32) for _ in range(nmax)]
    blob = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    t0 = time.perf_counter()
    exp = shim_shares(sk, sid, msgs)
    res = {"what": "batched BLS BN-P254 share signing, one signer, 32-byte messages",
           "reference": f"shim_sign_share on all {nmax} messages ({time.perf_counter() - t0:.1f} s), oracle samples",
           "quick": a.quick, "resources": RESOURCES, "batch": {}, "kernels": {}}

    hip = Hip()
    try:
        with cb.Context(device=0) as c:
            tid = c.load_bls_signers([sk], [sid])
            d_msg = hip.to_dev(blob)
            for n in sizes:
                off = np.arange(n, dtype=np.uint64) * np.uint64(32)
                lens = np.full(n, 32, dtype=np.uint32)
                out = np.zeros((n, 37), dtype=np.uint8)
                d_out = hip.to_dev(np.zeros(n * 37, dtype=np.uint8))

                def dev():
                    c.bls_sign_fixed_device(tid, 0, d_msg, 32, n, d_out, 0)
                    hip.sync()

                def host():
                    rc = c.lib.cbft_bls_sign_batch(c.handle, tid, None, _p(blob), _p(off), _p(lens), n, _p(out))
                    assert rc == 0, rc
                dev()
                check(f"device n={n}", hip.from_dev(d_out, n * 37).reshape(n, 37), exp[:n], sk, sid, msgs[:n], rng)
                host()
                check(f"host n={n}", out, exp[:n], sk, sid, msgs[:n], rng)
                res["batch"][str(n)] = {"device_resident": rate_entry(n, timed(dev, reps)),
                                        "host_arrays": rate_entry(n, timed(host, reps))}
                print(n, json.dumps(res["batch"][str(n)]), flush=True)

            # the one-message call, looped
            nl = 64 if a.quick else 256
            lone = [c.bls_sign(sk, sid, m) for m in msgs[:nl]]
            assert b"".join(lone) == exp[:nl].tobytes(), "cbft_bls_sign differs from the shim"
            ts = timed(lambda: [c.bls_sign(sk, sid, m) for m in msgs[:nl]], 3)
            res["lone_loop"] = rate_entry(nl, ts)
            print("lone", json.dumps(res["lone_loop"]), flush=True)

            # crossover: one batch call against n lone calls (host arrays both)
            cross = []
            for n in (1, 2, 4, 8, 16, 64):
                off = np.arange(n, dtype=np.uint64) * np.uint64(32)
                lens = np.full(n, 32, dtype=np.uint32)
                out = np.zeros((n, 37), dtype=np.uint8)

                def batch():
                    assert c.lib.cbft_bls_sign_batch(c.handle, tid, None, _p(blob), _p(off), _p(lens), n, _p(out)) == 0
                batch()
                assert out.tobytes() == exp[:n].tobytes()
                tb = statistics.median(timed(batch, 9))
                tl = statistics.median(timed(lambda: [c.bls_sign(sk, sid, m) for m in msgs[:n]], 5))
                cross.append({"n": n, "batch_call_ms": round(1e3 * tb, 4), "lone_calls_ms": round(1e3 * tl, 4)})
            res["crossover"] = cross
            res["crossover_n"] = next((r["n"] for r in cross if r["batch_call_ms"] < r["lone_calls_ms"]), None)
            print("crossover", json.dumps(cross), flush=True)
            c.unload_bls_signers(tid)
    finally:
        hip.close()

    # host build of the lane routine on 16 threads: a port of the GPU code, not RELIC
    nh = 512 if a.quick else 4096
    got, _ = lane_sign_many([(sk, sid)], [0] * nh, msgs[:nh], threads=16)
    assert got.tobytes() == exp[:nh].tobytes(), "host lane routine differs from the shim"
    ts = timed(lambda: lane_sign_many([(sk, sid)], [0] * nh, msgs[:nh], threads=16), 3)
    res["host_16_threads_port_not_RELIC"] = rate_entry(nh, ts)
    print("host", json.dumps(res["host_16_threads_port_not_RELIC"]), flush=True)

    # kernels: kept geometry and rejected variants, beside each other
    st = ctypes.CDLL(os.path.join(ROOT, "tests", "hip", "libbls_sign_selftest.so"))
    rec = np.zeros(12, dtype=np.uint32)
    sign_shim().bls_sign_shim_record(blsgen.be32(sk), sid, _p(rec))
    n = sizes[0]
    hb = (n + 255) // 256
    variants = (("stealing hash | window 3, LDS table (kept)", 1, 3, 1),
                ("plain hash loop | window 4, LDS table", 0, 4, 1),
                ("stealing hash | window 4, global table", 1, 4, 0))
    for name, steal, w, lds in variants + tuple((k + " (repeat)", s, w, l) for k, s, w, l in variants):
        out = np.zeros((n, 37), dtype=np.uint8)
        ms = np.zeros(2, dtype=np.float32)
        rounds = np.zeros(hb, dtype=np.uint32)
        rc = st.bls_sign_selftest_variant(steal, w, lds, _p(rec), _p(blob), 32, n, 3, _p(out), _p(ms), _p(rounds))
        assert rc == 0, rc
        assert out.tobytes() == exp[:n].tobytes(), f"{name}: shares differ from the shim"
        res["kernels"][name] = {
            "n": n, "hash_ms": round(float(ms[0]), 4), "mul_ms": round(float(ms[1]), 4),
            "hash_rounds_per_block_of_256_mean": round(float(rounds.mean()), 3),
            "hash_rounds_per_64_messages": round(float(rounds.mean()) / 4, 3),
            "hash_rounds_per_block_max": int(rounds.max())}
        print(name, json.dumps(res["kernels"][name]), flush=True)
    rec[:] = 0

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
