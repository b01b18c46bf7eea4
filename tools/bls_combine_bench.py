#!/usr/bin/env python3
"""Measures batched BLS share combination over many certificates and writes
profiles/bls_combine_batch.json.

One run, one GPU.  For every k one k-of-n Shamir sharing (oracle keygen, n = max(2k, 31)) and k of its
signers picked at random such that every Lagrange coefficient is a full-size value mod r (the general
case); certificate c is their k shares of its own 32-byte message, made on the GPU (cbft_bls_sign_batch,
pinned to the oracle by its own tests).
Any k shares of a degree-(k - 1) sharing combine to sk * g1_map(msg), and a multisig sum is
(sum sk_j) * g1_map(msg): every timed leg's outputs are first compared with those points for ALL its
certificates (signed under sk and under sum sk_j by the same signing call) and for a sample with the
Python oracle's own scalar multiplication; a mismatch aborts the run.  Legs:

  shapes      k = 3, 5, 9, 21, 67, 683, threshold and multisig, m from 1 up to 65,536 / k: one
              cbft_bls_combine_batch call (host arrays) and one cbft_bls_combine_fixed_device call
              (device-resident) against a loop of lone cbft_bls_combine calls over the same certificates
              (at most LONE_MAX of them: the loop's rate does not depend on m)
  crossover   one batch call against m lone calls, m = 1 .. 64, at k = 5, 3 and 21
              (k = 5 sets CBFT_BLS_COMBINE_BATCH_MIN_DEFAULT)
  tail        4,096 certificates of k = 5 with and without one k = 683 certificate among them
  stages      the four stages timed apart at about 64K shares, and the constant-time signing kernel on
              the same points (tests/hip/libbls_combine_selftest.so)

    python tools/bls_combine_bench.py [--out profiles/bls_combine_batch.json] [--quick]
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

LONE_MAX = 256

# registers / LDS / scratch per kernel as the compiler reports them for gfx950 (the .amdhsa_ lines of
# hipcc -S on csrc/bls_combine_batch.hip)
RESOURCES = {
    "blsc_decode_kernel": {"vgpr": 100, "agpr": 0, "scratch_bytes": 48, "lds_bytes": 0, "waves_per_simd": 4},
    "blsc_lagrange_kernel": {"vgpr": 98, "agpr": 0, "scratch_bytes": 0, "lds_bytes": 0, "waves_per_simd": 4},
    "blsc_mul_kernel": {"vgpr": 248, "agpr": 0, "scratch_bytes": 480, "lds_bytes": 27648, "waves_per_simd": 2},
    "blsc_wave_sum_kernel": {"vgpr": 248, "agpr": 0, "scratch_bytes": 336, "lds_bytes": 0, "waves_per_simd": 2},
    "blsc_finish_kernel": {"vgpr": 248, "agpr": 0, "scratch_bytes": 384, "lds_bytes": 0, "waves_per_simd": 2},
}


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def timed(f, reps, warm=0):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return ts


def entry(m, ts):
    med = statistics.median(ts)
    return {"m": m, "reps": len(ts), "ms_median": round(1e3 * med, 4), "ms_min": round(1e3 * min(ts), 4),
            "ms_max": round(1e3 * max(ts), 4), "certs_per_s_median": round(m / med, 1)}


class World:
    """mmax certificates of k shares: shares (mmax, k, 37) uint8 and the expected (mmax, 33) signatures,
    threshold and multisig."""

    def __init__(self, c, k, mmax, rng):
        self.k, self.m = k, mmax
        # k of n = max(2 k, 31) signers at random: with ids 1 .. k the coefficients would be small integers
        # (binomials), whose GLV halves are nearly all zero digits; most other subsets give fractions
        n = min(max(2 * k, 31), 2048)
        sk, sks = B.keygen(n, k, 0xC0B + k)
        # (full-size values mod r, the general case): an id set is drawn until every coefficient is one
        while True:
            self.ids = sorted(rng.sample(range(1, n + 1), k))
            if all(min(v, B.R - v) >> 200 for v in B.lagrange_coeffs(self.ids).values()):
                break
        ssum = sum(sks[i] for i in self.ids) % B.R
        self.msgs = [rng.randbytes(32) for _ in range(mmax)]
        tid = c.load_bls_signers([sks[i] for i in self.ids] + [sk, ssum], self.ids + [1, 1])
        try:
            per = max(1, 65536 // k)
            parts = []
            for lo in range(0, mmax, per):
                ms = self.msgs[lo:lo + per]
                parts.append(c.bls_sign_batch(tid, [m for m in ms for _ in range(k)], list(range(k)) * len(ms)).copy())
            self.shares = np.concatenate(parts).reshape(mmax, k, 37)
            self.want = {False: c.bls_sign_batch(tid, self.msgs, [k] * mmax)[:, 4:].copy(),
                         True: c.bls_sign_batch(tid, self.msgs, [k + 1] * mmax)[:, 4:].copy()}
        finally:
            c.unload_bls_signers(tid)
        for i in sorted({0, mmax - 1}):  # the signing kernel's points against the oracle's own products
            H = B.g1_map(self.msgs[i])
            assert self.want[False][i].tobytes() == B.g1_to_bytes(B.ec_mul(sk, H)), "signer vs oracle"
            assert self.want[True][i].tobytes() == B.g1_to_bytes(B.ec_mul(ssum, H)), "signer vs oracle"

    def check(self, name, out, status, m, multisig):
        if not (np.asarray(status)[:m] == 1).all():
            raise SystemExit(f"{name}: a certificate was refused")
        bad = np.nonzero((np.asarray(out).reshape(-1, 33)[:m] != self.want[multisig][:m]).any(axis=1))[0]
        if bad.size:
            raise SystemExit(f"{name}: {bad.size} of {m} certificates differ from sk * g1_map(msg), first {bad[:8]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bls_combine_batch.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes (a rehearsal, not a measurement)")
    a = ap.parse_args()
    total = 4096 if a.quick else 65536
    ks = [5, 67] if a.quick else [3, 5, 9, 21, 67, 683]
    reps, warm = (3, 1) if a.quick else (7, 2)
    cross_max = 8 if a.quick else 64
    rng = random.Random(0xC0B)
    res = {"what": "batched BLS BN-P254 share combination, k random signers of a k-of-max(2k,31) sharing, "
                   "full-size coefficients, one 32-byte message per certificate",
           "quick": a.quick, "resources": RESOURCES, "shapes": {}, "crossover": {}, "stages": {}}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    hip = Hip()
    worlds = {}
    try:
        with cb.Context(device=0) as c:
            for k in ks:
                mmax = max(1, total // k)
                w = worlds[k] = World(c, k, mmax, rng)
                flat = np.ascontiguousarray(w.shares.reshape(-1))
                d_sh = hip.to_dev(flat)
                ms_list = sorted({m for m in (1, 64, 4096, mmax) if m <= mmax})
                for multisig in (False, True):
                    kind = "multisig" if multisig else "threshold"
                    for m in ms_list:
                        off = np.arange(m + 1, dtype=np.uint64) * np.uint64(k)
                        out = np.zeros(33 * m, dtype=np.uint8)
                        st = np.zeros(m, dtype=np.uint8)
                        d_out, d_st = hip.to_dev(out), hip.to_dev(st)

                        def host():
                            assert c.lib.cbft_bls_combine_batch(c.handle, _p(flat), _p(off), m, None, int(multisig),
                                                                _p(out), _p(st)) == 0

                        def dev():
                            c.bls_combine_fixed_device(d_sh, k, m, 0, multisig, d_out, d_st, 0)
                            hip.sync()
                        nl = min(m, LONE_MAX)
                        certs = [[w.shares[i, j].tobytes() for j in range(k)] for i in range(nl)]
                        lone_out = []

                        def lone():
                            lone_out[:] = [c.bls_combine(s, multisig=multisig) for s in certs]
                        host()
                        w.check(f"host {kind} k={k} m={m}", out, st, m, multisig)
                        dev()
                        w.check(f"device {kind} k={k} m={m}", hip.from_dev(d_out, 33 * m), hip.from_dev(d_st, m), m, multisig)
                        lone()
                        w.check(f"lone {kind} k={k}", np.frombuffer(b"".join(lone_out), dtype=np.uint8), [1] * nl, nl, multisig)
                        e = {"k": k, "host_arrays": entry(m, timed(host, reps, warm)),
                             "device_resident": entry(m, timed(dev, reps, warm)),
                             "lone_loop": entry(nl, timed(lone, 3 if nl > 16 else reps, 1))}
                        e["batch_over_lone"] = round(e["host_arrays"]["certs_per_s_median"] /
                                                     e["lone_loop"]["certs_per_s_median"], 2)
                        res["shapes"][f"{kind}_k{k}_m{m}"] = e
                        print(kind, k, m, json.dumps(e), flush=True)
                write()

            # ---- crossover: one batch call against m lone calls (host arrays both)
            for k in [x for x in (5, 3, 21) if x in worlds]:
                w = worlds[k]
                rows = []
                for m in range(1, min(cross_max, w.m) + 1):
                    flat = np.ascontiguousarray(w.shares[:m].reshape(-1))
                    off = np.arange(m + 1, dtype=np.uint64) * np.uint64(k)
                    out = np.zeros(33 * m, dtype=np.uint8)
                    st = np.zeros(m, dtype=np.uint8)
                    certs = [[w.shares[i, j].tobytes() for j in range(k)] for i in range(m)]

                    def batch():
                        assert c.lib.cbft_bls_combine_batch(c.handle, _p(flat), _p(off), m, None, 0, _p(out), _p(st)) == 0
                    batch()
                    w.check(f"crossover k={k} m={m}", out, st, m, False)
                    tb = statistics.median(timed(batch, 7, 2))
                    tl = statistics.median(timed(lambda: [c.bls_combine(s) for s in certs], 5, 1))
                    rows.append({"m": m, "batch_call_ms": round(1e3 * tb, 4), "lone_calls_ms": round(1e3 * tl, 4)})
                wins = [r["batch_call_ms"] < r["lone_calls_ms"] for r in rows]
                first = next((i for i in range(len(rows)) if all(wins[i:])), None)
                res["crossover"][f"k{k}"] = {"rows": rows, "batch_wins_from_m": None if first is None else rows[first]["m"]}
                print("crossover", k, json.dumps(res["crossover"][f"k{k}"]["batch_wins_from_m"]), flush=True)
            write()

            # ---- the tail: one k = 683 certificate among 4,096 of k = 5
            if 5 in worlds and 683 in worlds:
                w5, wl = worlds[5], worlds[683]
                m5 = min(4096, w5.m)
                small = [w5.shares[i].reshape(-1) for i in range(m5)]
                mid = m5 // 2
                flat_a = np.ascontiguousarray(np.concatenate(small))
                flat_b = np.ascontiguousarray(np.concatenate(small[:mid] + [wl.shares[0].reshape(-1)] + small[mid:]))
                off_a = np.arange(m5 + 1, dtype=np.uint64) * np.uint64(5)
                lens = [5] * mid + [683] + [5] * (m5 - mid)
                off_b = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
                out = np.zeros(33 * (m5 + 1), dtype=np.uint8)
                st = np.zeros(m5 + 1, dtype=np.uint8)

                def run_a():
                    assert c.lib.cbft_bls_combine_batch(c.handle, _p(flat_a), _p(off_a), m5, None, 0, _p(out), _p(st)) == 0

                def run_b():
                    assert c.lib.cbft_bls_combine_batch(c.handle, _p(flat_b), _p(off_b), m5 + 1, None, 0, _p(out), _p(st)) == 0
                run_b()
                got = out.reshape(-1, 33)
                assert st.all() and (got[mid] == wl.want[False][0]).all(), "tail: the large certificate is wrong"
                assert (np.delete(got, mid, axis=0) == w5.want[False][:m5]).all(), "tail: a small certificate is wrong"
                ta, tb = [], []
                for _ in range(reps + warm):
                    ta += timed(run_a, 1)
                    tb += timed(run_b, 1)
                res["tail"] = {"m_small": m5, "without_large": entry(m5, ta[warm:]), "with_one_k683": entry(m5 + 1, tb[warm:])}
                print("tail", json.dumps(res["tail"]), flush=True)
                write()
    finally:
        hip.close()

    # ---- the stages timed apart (best of 3) at about 64K shares
    st_lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hip", "libbls_combine_selftest.so"))
    for k in [x for x in (5, 21, 683) if x in worlds]:
        w = worlds[k]
        m = w.m
        for multisig in (False, True):
            flat = np.ascontiguousarray(w.shares.reshape(-1))
            out = np.zeros(33 * m, dtype=np.uint8)
            st = np.zeros(m, dtype=np.uint8)
            ms = np.zeros(6, dtype=np.float32)
            rc = st_lib.blsc_selftest_run(_p(flat), k, m, int(multisig), _p(out), _p(st), 3, _p(ms))
            assert rc == 0, rc
            w.check(f"stages k={k}", out, st, m, multisig)
            kind = "multisig" if multisig else "threshold"
            res["stages"][f"{kind}_k{k}"] = {
                "k": k, "m": m, "shares": m * k, "batch_ms": round(float(ms[0]), 4), "decode_ms": round(float(ms[1]), 4),
                "lagrange_ms": round(float(ms[2]), 4), "mul_ms": round(float(ms[3]), 4), "sum_close_ms": round(float(ms[4]), 4),
                "ct_sign_mul_kernel_ms": round(float(ms[5]), 4)}
            print("stages", kind, json.dumps(res["stages"][f"{kind}_k{k}"]), flush=True)
    write()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
