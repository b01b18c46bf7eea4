#!/usr/bin/env python3
"""Measures batched BLS multisig verification over many signer sets and writes
profiles/bls_multisig_verify_batch.json.

One run, one GPU.  A multisig certificate under signer set S is (sum of sk_i over S) * H(m), so the
certificates are made on the GPU by cbft_bls_sign_batch under the summed secrets (pinned to the oracle by
its own tests).  Every 16th item of every leg names another message and must fail; every timed leg's
verdicts are compared with that construction first and 16 sampled items with the lone
cbft_bls_verify_multisig; a mismatch aborts the run.  Two key-set shapes, n = 16 / k = 11 (production) and
n = 1,024 / k = 683 (SURVEY config #4), each with every item naming one set, 16 sets cycling, and every
item naming its own set entry (the entries are drawn from 256 distinct bitmaps: the C call does not merge
equal bitmaps, so each entry is summed and its lines are built).  Legs:

  batch       cbft_bls_verify_multisig_fixed_device (device-resident) and cbft_bls_verify_multisig_batch
              (host arrays in, bitmap out) at 65,536 and 4,096 items
  ceiling     cbft_bls_verify_fixed_device / cbft_bls_verify_batch under slot 0 at the same n: the same
              pairing work with no key sum and no line computation
  lone        a loop of cbft_bls_verify_multisig over 256 certificates (the rate before this entry)
  sums        cbft_bls_sum_keys_batch alone at 4,096 sets
  crossover   one batch call against n lone calls, n = 1 .. 64, every item its own set entry
              (sets CBFT_BLS_MULTISIG_BATCH_MIN_DEFAULT from the production shape)

    python tools/bls_multisig_verify_bench.py [--out profiles/bls_multisig_verify_batch.json] [--quick]
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

import bn254_ref as B  # noqa: E402
import cbft_hipcrypto as cb  # noqa: E402
from sign_vectors import Hip  # noqa: E402

SHAPES = {"n16_k11": (16, 11), "n1024_k683": (1024, 683)}
NOWN = 256  # distinct bitmaps behind the "own set" entries

# registers / LDS / scratch per kernel as the compiler reports them for gfx950 (the .amdhsa_ lines of
# hipcc -S on csrc/bls_multisig_batch.hip); the decode, hash and pairing kernels are those of
# csrc/bls_verify_batch.hip (tools/bls_verify_bench.py)
RESOURCES = {
    "blsm_sum_part_kernel": {"vgpr": 66, "agpr": 0, "scratch_bytes": 0, "lds_bytes": 0, "waves_per_simd": 7},
    "blsm_sum_fin_kernel": {"vgpr": 229, "agpr": 0, "scratch_bytes": 544, "lds_bytes": 220, "waves_per_simd": 2},
    "blsm_lines_kernel": {"vgpr": 244, "agpr": 0, "scratch_bytes": 288, "lds_bytes": 20160, "waves_per_simd": 2},
    "blsm_ident_kernel": {"vgpr": 4, "agpr": 0, "scratch_bytes": 0, "lds_bytes": 0, "waves_per_simd": 8},
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


def rate_entry(n, ts, **extra):
    med = statistics.median(ts)
    e = {"n": n, "reps": len(ts), "ms_median": round(1e3 * med, 4), "ms_min": round(1e3 * min(ts), 4),
         "ms_max": round(1e3 * max(ts), 4), "us_per_item_median": round(1e6 * med / n, 4),
         "items_per_s_median": round(n / med, 1)}
    e.update(extra)
    return e


def must_equal(name, got, exp):
    got, exp = np.asarray(got).astype(bool), np.asarray(exp).astype(bool)
    bad = np.nonzero(got != exp)[0]
    if bad.size:
        raise SystemExit(f"{name}: {bad.size} of {exp.size} verdicts differ from the construction, first {bad[:8]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bls_multisig_verify_batch.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal, not a measurement)")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    sizes = [1024, 256] if a.quick else [65536, 4096]
    reps = 3 if a.quick else 7
    ncert = 32 if a.quick else 256
    nsum = 256 if a.quick else 4096
    ncross = 8 if a.quick else 64
    nmax = max(sizes)
    rng = random.Random(0xB25)
    msgs = [rng.randbytes(32) for _ in range(nmax)]
    blob = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    idx = np.arange(nmax)
    exp = idx % 16 != 5
    res = {"what": "batched BLS BN-P254 multisig verification, 32-byte messages, every 16th item invalid",
           "quick": a.quick, "resources": RESOURCES, "shapes": {}}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    hip = Hip()
    try:
        with cb.Context(device=0) as c:
            d_msg = hip.to_dev(blob)
            for shape in a.shapes.split(","):
                nk, k = SHAPES[shape]
                sks = [rng.randrange(1, B.R) for _ in range(nk)]
                sk0 = rng.randrange(1, B.R)
                # signer sets: 16 that cycle (set 0 is also the "one set"), and NOWN more: a base set with
                # one signer swapped for one outside it
                cyc = [sorted(rng.sample(range(1, nk + 1), k)) for _ in range(16)]
                base = sorted(rng.sample(range(1, nk + 1), k))
                outside = [i for i in range(1, nk + 1) if i not in base]
                own = []
                while len(own) < NOWN:
                    x, y = rng.choice(base), rng.choice(outside)
                    own.append(sorted([i for i in base if i != x] + [y]))
                allsets = cyc + own
                sums = [sum(sks[i - 1] for i in s) % B.R for s in allsets]
                maps = [B.signers_bitmap(s) for s in allsets]
                tid = c.load_bls_signers(sks, list(range(1, nk + 1)))
                vks = c.bls_signer_public_keys(tid)
                c.unload_bls_signers(tid)
                tid = c.load_bls_signers(sums + [sk0], [1] * (len(sums) + 1))
                modes = {
                    "one_set": np.zeros(nmax, dtype=np.uint32),
                    "sets_16": (idx % 16).astype(np.uint32),
                    "own_set": (16 + idx % NOWN).astype(np.uint32),  # index into allsets
                }
                sig = {m: c.bls_sign_batch(tid, msgs, so.tolist())[:, 4:].copy() for m, so in modes.items()}
                sig0 = c.bls_sign_batch(tid, msgs, [len(sums)] * nmax)[:, 4:].copy()
                c.unload_bls_signers(tid)
                kid = c.bls_load_keys(c.bls_public_key(sk0), vks)
                assert all(c.bls_key_status(kid, nk))
                mof = np.where(exp, idx, (idx + 1) % 256).astype(np.uint32)  # every 16th names another message
                out = res["shapes"][shape] = {"n_keys": nk, "k": k, "batch": {}, "ceiling": {}}

                for n in sizes:
                    mo = np.ascontiguousarray(mof[:n])
                    d_mo = hip.to_dev(mo)
                    off = np.arange(n, dtype=np.uint64) * np.uint64(32)
                    lens = np.full(n, 32, dtype=np.uint32)
                    bits = np.zeros((n + 7) // 8, dtype=np.uint8)
                    d_valid = hip.to_dev(np.zeros(n, dtype=np.uint8))
                    for mode, so in modes.items():
                        sg = np.ascontiguousarray(sig[mode][:n])
                        if mode == "own_set":  # one entry per item
                            sets = np.frombuffer(b"".join(maps[j] for j in so[:n]), dtype=np.uint8).copy()
                            s, sof = n, None
                        elif mode == "sets_16":
                            sets = np.frombuffer(b"".join(maps[:16]), dtype=np.uint8).copy()
                            s, sof = 16, np.ascontiguousarray(so[:n])
                        else:
                            sets = np.frombuffer(maps[0], dtype=np.uint8).copy()
                            s, sof = 1, np.ascontiguousarray(so[:n])
                        d_sets, d_sig = hip.to_dev(sets), hip.to_dev(sg.reshape(-1))
                        d_sof = 0 if sof is None else hip.to_dev(sof)

                        def dev():
                            c.bls_verify_multisig_fixed_device(kid, d_sets, s, d_sof, d_sig, d_msg, 32, n, d_mo, n,
                                                               d_valid, 0)
                            hip.sync()

                        def host():
                            assert c.lib.cbft_bls_verify_multisig_batch(c.handle, kid, _p(sets), s, _p(sof), _p(sg),
                                                                        _p(blob), _p(off), _p(lens), n, _p(mo), n,
                                                                        _p(bits)) == 0
                        dev()
                        got = hip.from_dev(d_valid, n)
                        must_equal(f"{shape} device {mode} n={n}", got, exp[:n])
                        host()
                        must_equal(f"{shape} host {mode} n={n}", cb.bitmap_to_bools(bits.tobytes(), n), exp[:n])
                        for i in rng.sample(range(n), 16):  # against the lone call: an independent kernel
                            lone = c.bls_verify_multisig(kid, msgs[int(mo[i])], sg[i].tobytes(), maps[int(so[i])])
                            if bool(lone) != bool(got[i]):
                                raise SystemExit(f"{shape} {mode} n={n}: item {i} differs from cbft_bls_verify_multisig")
                        out["batch"][f"{mode}_{n}"] = {"sets": s, "device_resident": rate_entry(n, timed(dev, reps)),
                                                      "host_arrays": rate_entry(n, timed(host, reps))}
                        print(shape, mode, n, json.dumps(out["batch"][f"{mode}_{n}"]), flush=True)
                    # the ceiling: the same items under slot 0 of the key set
                    sg = np.ascontiguousarray(sig0[:n])
                    d_sig = hip.to_dev(sg.reshape(-1))

                    def cdev():
                        c.bls_verify_fixed_device(kid, 0, d_sig, d_msg, 32, n, d_mo, n, d_valid, 0)
                        hip.sync()

                    def chost():
                        assert c.lib.cbft_bls_verify_batch(c.handle, kid, None, _p(sg), _p(blob), _p(off), _p(lens), n,
                                                           _p(mo), n, _p(bits)) == 0
                    cdev()
                    must_equal(f"{shape} ceiling n={n}", hip.from_dev(d_valid, n), exp[:n])
                    out["ceiling"][str(n)] = {"device_resident": rate_entry(n, timed(cdev, reps)),
                                              "host_arrays": rate_entry(n, timed(chost, reps))}
                    print(shape, "ceiling", n, json.dumps(out["ceiling"][str(n)]), flush=True)

                # ---- the one-certificate call, looped over the 16 cycling sets
                csig = [sig["sets_16"][i].tobytes() for i in range(ncert)]
                assert all(c.bls_verify_multisig(kid, msgs[i], csig[i], maps[i % 16]) for i in range(ncert))
                assert not c.bls_verify_multisig(kid, msgs[1], csig[0], maps[0])
                out["lone_loop"] = rate_entry(ncert, timed(lambda: [c.bls_verify_multisig(kid, msgs[i], csig[i], maps[i % 16])
                                                                    for i in range(ncert)], 3))
                print(shape, "lone", json.dumps(out["lone_loop"]), flush=True)

                # ---- the key sums alone
                some = [maps[16 + j % NOWN] for j in range(nsum)]
                got65, ok = c.bls_sum_keys_batch(kid, some)
                assert ok.all() and all(got65[j] == c.bls_sum_keys(kid, some[j]) for j in rng.sample(range(nsum), 8))
                out["sum_keys_batch"] = rate_entry(nsum, timed(lambda: c.bls_sum_keys_batch(kid, some), reps))
                out["sum_keys_lone_loop"] = rate_entry(64, timed(lambda: [c.bls_sum_keys(kid, some[j]) for j in range(64)], 3))
                print(shape, "sums", json.dumps(out["sum_keys_batch"]), json.dumps(out["sum_keys_lone_loop"]), flush=True)

                # ---- crossover: one batch call against n lone calls (host arrays both), own set entries
                cross = []
                so = modes["own_set"]
                for n in range(1, ncross + 1):
                    off = np.arange(n, dtype=np.uint64) * np.uint64(32)
                    lens = np.full(n, 32, dtype=np.uint32)
                    bits = np.zeros((n + 7) // 8, dtype=np.uint8)
                    sg = np.ascontiguousarray(sig["own_set"][:n])
                    sets = np.frombuffer(b"".join(maps[j] for j in so[:n]), dtype=np.uint8).copy()
                    osig = [sg[i].tobytes() for i in range(n)]

                    def batch():
                        assert c.lib.cbft_bls_verify_multisig_batch(c.handle, kid, _p(sets), n, None, _p(sg), _p(blob),
                                                                    _p(off), _p(lens), n, None, n, _p(bits)) == 0
                    batch()
                    must_equal(f"{shape} crossover n={n}", cb.bitmap_to_bools(bits.tobytes(), n), np.ones(n, dtype=bool))
                    tb = statistics.median(timed(batch, 7))
                    tl = statistics.median(timed(lambda: [c.bls_verify_multisig(kid, msgs[i], osig[i], maps[int(so[i])])
                                                          for i in range(n)], 5))
                    cross.append({"n": n, "batch_call_ms": round(1e3 * tb, 4), "lone_calls_ms": round(1e3 * tl, 4)})
                out["crossover"] = cross
                # the smallest n from which the batch call wins at every larger n of the table
                win = [r["batch_call_ms"] < r["lone_calls_ms"] for r in cross]
                out["crossover_n"] = next((cross[i]["n"] for i in range(len(cross)) if all(win[i:])), None)
                print(shape, "crossover", out["crossover_n"], json.dumps(cross), flush=True)
                c.bls_unload_keys(kid)
                write()
    finally:
        hip.close()
    write()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
