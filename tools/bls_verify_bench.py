#!/usr/bin/env python3
"""Measures batched BLS verification over many messages and writes
profiles/bls_verify_batch.json.

One run, one GPU.  Shares and combined signatures are made on the GPU (cbft_bls_sign_batch, pinned to the
oracle by its own tests); every 16th item of every leg is spoiled (checked under another key slot) and
every timed leg's verdicts are compared with that construction first, a sample with the lone calls; a
mismatch aborts the run.  Legs:

  per_item    the parent's throughput form (cbft_bls_verify_shares, k = 2,048 shares of ONE message)
              alternated with the batch at n = 2,048 DISTINCT messages: the same pairing work per item
              plus one hash per message
  batch       cbft_bls_verify_fixed_device (device-resident) and cbft_bls_verify_batch (host arrays in,
              bitmap out) at 65,536 and 4,096 items, with distinct messages and with m = n / 683 messages
              (a collector's shape)
  lone        a loop of cbft_bls_verify over 256 certificates (the rate before this entry existed)
  crossover   one batch call against n lone cbft_bls_verify calls, n = 1 .. 64
              (sets CBFT_BLS_VERIFY_BATCH_MIN_DEFAULT)
  stages      the decode, hash and pairing kernels of the batch timed apart
              (tests/hip/libbls_verify_selftest.so)

    python tools/bls_verify_bench.py [--out profiles/bls_verify_batch.json] [--quick]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("concord-bft_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import blsgen  # noqa: E402
import cbft_hipcrypto as cb  # noqa: E402
from sign_vectors import Hip  # noqa: E402

NKEYS, THRESH = 16, 11

# registers / LDS / scratch per kernel as the compiler reports them for gfx950 (the .amdhsa_ lines of
# hipcc -S on csrc/bls_verify_batch.hip and csrc/bls_pairing.hip)
RESOURCES = {
    "blsv_pair_kernel": {"vgpr": 256, "agpr": 36, "scratch_bytes": 124, "lds_bytes": 30240, "waves_per_simd": 1},
    "bls_share_verify_kernel<1> (the yardstick)": {"vgpr": 256, "agpr": 39, "scratch_bytes": 124, "lds_bytes": 30240,
                                                   "waves_per_simd": 1},
    "blsv_decode_kernel": {"vgpr": 100, "agpr": 0, "scratch_bytes": 48, "lds_bytes": 0, "waves_per_simd": 4},
    "bls_sign_hash_kernel<steal> (this object)": {"vgpr": 256, "agpr": 24, "scratch_bytes": 768, "lds_bytes": 4,
                                                  "waves_per_simd": 1},
}


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def timed(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return ts


def rate_entry(n, ts, m=None):
    med = statistics.median(ts)
    e = {"n": n, "reps": len(ts), "ms_median": round(1e3 * med, 4), "ms_min": round(1e3 * min(ts), 4),
         "ms_max": round(1e3 * max(ts), 4), "us_per_item_median": round(1e6 * med / n, 4),
         "items_per_s_median": round(n / med, 1)}
    if m is not None:
        e["m"] = m
    return e


def must_equal(name, got, exp):
    got, exp = np.asarray(got).astype(bool), np.asarray(exp).astype(bool)
    bad = np.nonzero(got != exp)[0]
    if bad.size:
        raise SystemExit(f"{name}: {bad.size} of {exp.size} verdicts differ from the construction, first {bad[:8]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bls_verify_batch.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal, not a measurement)")
    a = ap.parse_args()
    sizes = [1024, 256] if a.quick else [65536, 4096]
    nyard = 256 if a.quick else 2048
    reps = 3 if a.quick else 7
    per_msg = 64 if a.quick else 683
    rng = random.Random(0xB20)
    nmax = max(sizes)
    sk, sks, pk, vks = blsgen.keyset(NKEYS, THRESH, seed=0xB21)
    msgs = [rng.randbytes(32) for _ in range(nmax)]
    blob = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    mcol = (nmax + per_msg - 1) // per_msg
    ncert = 64 if a.quick else 256
    res = {"what": "batched BLS BN-P254 verification, 16-signer key set, 32-byte messages, every 16th item invalid",
           "quick": a.quick, "resources": RESOURCES, "batch": {}, "stages": {}}

    hip = Hip()
    try:
        with cb.Context(device=0) as c:
            # signer table: the 16 share keys and the group secret (its "share" is the combined signature)
            tid = c.load_bls_signers([sks[i] for i in range(1, NKEYS + 1)] + [sk], list(range(1, NKEYS + 1)) + [1])
            own = c.bls_sign_batch(tid, msgs, [i % NKEYS for i in range(nmax)])[:, 4:].copy()
            grid = c.bls_sign_batch(tid, [msgs[j] for j in range(mcol) for _ in range(NKEYS)],
                                    [s for _ in range(mcol) for s in range(NKEYS)])[:, 4:].copy()
            cert = c.bls_sign_batch(tid, msgs[:ncert], [NKEYS] * ncert)[:, 4:].copy()
            c.unload_bls_signers(tid)
            kid = c.bls_load_keys(pk, vks)
            assert all(c.bls_key_status(kid, NKEYS))

            idx = np.arange(nmax)
            exp = idx % 16 != 5
            slot = np.where(exp, idx % NKEYS + 1, (idx + 1) % NKEYS + 1).astype(np.uint32)
            # collector's shape: item i is signer i % 16's share of message i // per_msg
            col_sig = np.ascontiguousarray(grid[(idx // per_msg) * NKEYS + idx % NKEYS])
            col_of = (idx // per_msg).astype(np.uint32)

            # ---- per-item time against the parent's throughput form, alternated
            shares1 = b"".join((s + 1).to_bytes(4, "big") + grid[s].tobytes() for s in (i % NKEYS for i in range(nyard)))
            bm = ctypes.create_string_buffer((nyard + 7) // 8)
            off = np.arange(nyard, dtype=np.uint64) * np.uint64(32)
            lens = np.full(nyard, 32, dtype=np.uint32)
            out = np.zeros((nyard + 7) // 8, dtype=np.uint8)
            sig_y = np.ascontiguousarray(own[:nyard])
            slot_y = np.ascontiguousarray(slot[:nyard])

            def yard():
                assert c.lib.cbft_bls_verify_shares(c.handle, kid, msgs[0], 32, shares1, nyard, bm) == 0

            def batch_y():
                assert c.lib.cbft_bls_verify_batch(c.handle, kid, _p(slot_y), _p(sig_y), _p(blob), _p(off), _p(lens),
                                                   nyard, None, nyard, _p(out)) == 0
            yard()
            must_equal("yardstick", cb.bitmap_to_bools(bm.raw, nyard), np.ones(nyard, dtype=bool))
            batch_y()
            must_equal("batch 2048", cb.bitmap_to_bools(out.tobytes(), nyard), exp[:nyard])
            ty, tb = [], []
            for _ in range(reps):
                ty += timed(yard, 1)
                tb += timed(batch_y, 1)
            res["per_item"] = {"yardstick_verify_shares_one_message": rate_entry(nyard, ty),
                               "batch_distinct_messages": rate_entry(nyard, tb, nyard)}
            print("per_item", json.dumps(res["per_item"]), flush=True)

            # ---- rates at scale
            d_msg = hip.to_dev(blob)
            for n in sizes:
                for shape in ("distinct", "collector"):
                    m = n if shape == "distinct" else (n + per_msg - 1) // per_msg
                    sg = np.ascontiguousarray(own[:n] if shape == "distinct" else col_sig[:n])
                    mo = None if shape == "distinct" else np.ascontiguousarray(col_of[:n])
                    sl = np.ascontiguousarray(slot[:n])
                    off = np.arange(m, dtype=np.uint64) * np.uint64(32)
                    lens = np.full(m, 32, dtype=np.uint32)
                    out = np.zeros((n + 7) // 8, dtype=np.uint8)
                    d_sig, d_slot = hip.to_dev(sg.reshape(-1)), hip.to_dev(sl)
                    d_of = 0 if mo is None else hip.to_dev(mo)
                    d_valid = hip.to_dev(np.zeros(n, dtype=np.uint8))

                    def dev():
                        c.bls_verify_fixed_device(kid, d_slot, d_sig, d_msg, 32, m, d_of, n, d_valid, 0)
                        hip.sync()

                    def host():
                        assert c.lib.cbft_bls_verify_batch(c.handle, kid, _p(sl), _p(sg), _p(blob), _p(off), _p(lens), m,
                                                           _p(mo), n, _p(out)) == 0
                    dev()
                    got = hip.from_dev(d_valid, n)
                    must_equal(f"device {shape} n={n}", got, exp[:n])
                    host()
                    must_equal(f"host {shape} n={n}", cb.bitmap_to_bools(out.tobytes(), n), exp[:n])
                    for i in rng.sample(range(n), 16):  # against the lone call: an independent kernel
                        j = int(mo[i]) if mo is not None else i
                        lone = c.bls_verify_shares(kid, msgs[j], [int(sl[i]).to_bytes(4, "big") + sg[i].tobytes()])[0]
                        if bool(lone) != bool(got[i]):
                            raise SystemExit(f"{shape} n={n}: item {i} differs from cbft_bls_verify_shares")
                    res["batch"][f"{shape}_{n}"] = {"device_resident": rate_entry(n, timed(dev, reps), m),
                                                    "host_arrays": rate_entry(n, timed(host, reps), m)}
                    print(shape, n, json.dumps(res["batch"][f"{shape}_{n}"]), flush=True)

            # ---- the one-certificate call, looped
            csig = [cert[i].tobytes() for i in range(ncert)]
            assert all(c.bls_verify(kid, msgs[i], csig[i]) for i in range(ncert)), "cbft_bls_verify rejects a certificate"
            assert not c.bls_verify(kid, msgs[1], csig[0])
            res["lone_loop"] = rate_entry(ncert, timed(lambda: [c.bls_verify(kid, msgs[i], csig[i])
                                                                for i in range(ncert)], 3))
            print("lone", json.dumps(res["lone_loop"]), flush=True)

            # ---- crossover: one batch call against n lone calls (host arrays both, slot 0)
            cross = []
            for n in range(1, (16 if a.quick else 64) + 1):
                off = np.arange(n, dtype=np.uint64) * np.uint64(32)
                lens = np.full(n, 32, dtype=np.uint32)
                out = np.zeros((n + 7) // 8, dtype=np.uint8)
                sg = np.ascontiguousarray(cert[:n])

                def batch():
                    assert c.lib.cbft_bls_verify_batch(c.handle, kid, None, _p(sg), _p(blob), _p(off), _p(lens), n, None, n,
                                                       _p(out)) == 0
                batch()
                must_equal(f"crossover n={n}", cb.bitmap_to_bools(out.tobytes(), n), np.ones(n, dtype=bool))
                tb = statistics.median(timed(batch, 7))
                tl = statistics.median(timed(lambda: [c.bls_verify(kid, msgs[i], csig[i]) for i in range(n)], 5))
                cross.append({"n": n, "batch_call_ms": round(1e3 * tb, 4), "lone_calls_ms": round(1e3 * tl, 4)})
            res["crossover"] = cross
            res["crossover_n"] = next((r["n"] for r in cross if r["batch_call_ms"] < r["lone_calls_ms"]), None)
            print("crossover", json.dumps(cross), flush=True)
            c.bls_unload_keys(kid)
    finally:
        hip.close()

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    write()
    # ---- the batch's kernels timed apart (best of 3), at the yardstick's size and at the largest
    st = ctypes.CDLL(os.path.join(ROOT, "tests", "hip", "libbls_verify_selftest.so"))
    keys = np.frombuffer(pk + b"".join(vks), dtype=np.uint8).copy()
    for n in sorted({nyard, sizes[0]}):
        got = np.zeros(n, dtype=np.uint8)
        ms = np.zeros(4, dtype=np.float32)
        sl, sg = np.ascontiguousarray(slot[:n]), np.ascontiguousarray(own[:n])
        rc = st.blsv_selftest_run(_p(keys), NKEYS, _p(sl), None, _p(sg), _p(blob), 32, n, n, _p(got), 3, _p(ms))
        assert rc == 0, rc
        must_equal(f"stages n={n}", got, exp[:n])
        res["stages"][str(n)] = {"n": n, "m": n, "batch_ms": round(float(ms[0]), 4), "decode_ms": round(float(ms[1]), 4),
                                 "hash_ms": round(float(ms[2]), 4), "pair_ms": round(float(ms[3]), 4),
                                 "pair_us_per_item": round(1e3 * float(ms[3]) / n, 4)}
        print("stages", json.dumps(res["stages"][str(n)]), flush=True)
        write()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
