#!/usr/bin/env python3
"""ECDSA P-256 / SHA-256 batch verification on one GPU against the host OpenSSL, with the secp256k1 batch of
the same size beside it, in one run.

    python3 tools/ecdsa_p256_bench.py [--out profiles/ecdsa_p256_verify.json] [--threads 16]

Sizes: 4,096, 65,536 and 262,144 signatures over 256-byte messages and 4,096 keys, one in a hundred damaged.
Modes: device-resident arrays (cbft_ecdsa_verify_batch_device on a P-256 table, wall time to a synchronised
stream and the kernels' own time from cbft_ecdsa_kernel_ms; two warm runs, then the median of 7) and host arrays
(cbft_ecdsa_verify_batch, copies included; median of 5).  The same run times cbft_ecdsa_verify_batch on a
secp256k1 table at the same n and `threads` host threads of SHA256 + ECDSA_do_verify on prime256v1 with cached
EC_KEYs (tools/cpu_baseline/openssl_ecdsa_p256.c), whose verdicts are also the expected ones: every GPU verdict
of every timed run is compared with them.  Last, the crossover: the smallest power of two n at which one
host-array call's median is below a one-thread OpenSSL P-256 loop's median, n = 1 .. 4,096, extended to 16,384
when it is not reached.  The box is named in the output.

MAD64 fraction: executed v_mad_u64_u32 per verification x n / kernel time / 39.32e12.  The count is 66 per field
product (the ISA listing of the kept reduction, `make p256_isa`) times the products a verification with random
scalars runs: 64 windows x (4 doublings x 8 + 2 x 15/16 mixed additions x 11) + 3 for the closing comparison,
plus 3 x 128 for the three Montgomery products mod n.
"""
import argparse
import ctypes
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("concord-bft_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (initialises HIP before the library does)

import cbft_hipcrypto as cb  # noqa: E402

CPU_DIR = os.path.join(ROOT, "tools", "cpu_baseline")
MAD64_PEAK = 39.32e12
MAD64_PER_FE_MUL = 66
FE_MUL_PER_VERIFY = 64 * (4 * 8 + 2 * 15 / 16 * 11) + 3
MAD64_PER_VERIFY = MAD64_PER_FE_MUL * FE_MUL_PER_VERIFY + 3 * 128
NKEYS = 4096
MSG_LEN = 256
SIZES = (4096, 65536, 262144)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Cpu:
    """One of the two host baselines: prefix cbft_cpu_p256_ (prime256v1) or cbft_cpu_ecdsa_ (secp256k1)."""

    def __init__(self, so, prefix):
        self.lib = ctypes.CDLL(os.path.join(CPU_DIR, so))
        f = lambda name: getattr(self.lib, prefix + name)  # noqa: E731
        self.keys_new, self.keys_free, self.verify_, self.keygen_, self.sign_ = (
            f("keys_new"), f("keys_free"), f("verify"), f("keygen"), f("sign_many"))
        self.keys_new.restype = ctypes.c_void_p
        self.keys_new.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        self.keys_free.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        self.verify_.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
        self.keygen_.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        self.sign_.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4 + [
            ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]

    def keygen(self, nkeys):
        priv, pub = np.zeros(nkeys * 32, np.uint8), np.zeros(nkeys * 64, np.uint8)
        assert self.keygen_(nkeys, _p(priv), _p(pub)) == 0
        return priv, pub

    def sign(self, priv, nkeys, kidx, blob, off, ln, threads):
        sig = np.zeros(len(kidx) * 64, np.uint8)
        assert self.sign_(_p(priv), nkeys, _p(kidx), _p(blob), _p(off), _p(ln), len(kidx), _p(sig), threads) == 0
        return sig

    def verify(self, cache, kidx, sig, blob, off, ln, n, threads):
        out = np.zeros(n, np.uint8)
        t0 = time.perf_counter()
        self.verify_(cache, _p(kidx), _p(sig), _p(blob), _p(off), _p(ln), n, _p(out), threads)
        return time.perf_counter() - t0, out.astype(bool)


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def words_to_bools(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def host_call(ctx, tid, kidx, sig, blob, off, ln, n, bitmap):
    bitmap[:] = 0xFF
    t0 = time.perf_counter()
    rc = ctx.lib.cbft_ecdsa_verify_batch(ctx.handle, tid, _p(kidx), _p(sig), _p(blob), _p(off), _p(ln), n, _p(bitmap))
    dt = time.perf_counter() - t0
    assert rc == 0
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecdsa_p256_verify.json"))
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    args = ap.parse_args()

    cpu = Cpu("libcbft_cpu_openssl_ecdsa_p256.so", "cbft_cpu_p256_")
    cpu_k1 = Cpu("libcbft_cpu_openssl_ecdsa.so", "cbft_cpu_ecdsa_")
    rng = np.random.default_rng(0x9256)
    nmax = max(max(args.sizes), 16384)
    kidx = rng.integers(0, NKEYS, nmax, dtype=np.uint32)
    blob = rng.integers(0, 256, nmax * MSG_LEN, dtype=np.uint8)
    off = (np.arange(nmax, dtype=np.uint64) * MSG_LEN)
    ln = np.full(nmax, MSG_LEN, dtype=np.uint32)
    bad = np.arange(37, nmax, 100)

    def inputs(c):
        priv, pub = c.keygen(NKEYS)
        sig = c.sign(priv, NKEYS, kidx, blob, off, ln, args.threads)
        sig[bad * 64 + (bad % 64)] ^= np.uint8(1) << (bad % 8).astype(np.uint8)  # one bit of r or s
        return pub, sig, c.keys_new(_p(pub), NKEYS)

    pub, sig, cache = inputs(cpu)
    pub_k1, sig_k1, cache_k1 = inputs(cpu_k1)

    torch.zeros(1, device="cuda:0")
    dev = torch.device("cuda:0")
    result = {
        "what": "ECDSA P-256 / SHA-256 batch verification, one GPU against host OpenSSL threads, with the secp256k1 "
                "batch of the same size beside it, one run",
        "box": {"gpu": torch.cuda.get_device_name(0), "host_cpu": platform.processor() or platform.machine(),
                "torch": torch.__version__, "hip": getattr(torch.version, "hip", None)},
        "workload": {"keys": NKEYS, "msg_len": MSG_LEN, "damaged": "1 in 100 (one bit of r or s)"},
        "cpu_threads": args.threads, "mad64_per_verify": MAD64_PER_VERIFY, "sizes": [],
    }
    try:
        with open("/proc/cpuinfo") as f:
            names = [line.split(":", 1)[1].strip() for line in f if line.startswith("model name")]
        if names:
            result["box"]["host_cpu"] = names[0]
    except OSError:
        pass

    with cb.Context(0) as ctx:
        tid = ctx.ecdsa_load_keys(pub.reshape(-1, 64), curve="p256")
        tid_k1 = ctx.ecdsa_load_keys(pub_k1.reshape(-1, 64))
        assert ctx.ecdsa_key_status(tid, NKEYS).all() and ctx.ecdsa_key_status(tid_k1, NKEYS).all()
        d_k = torch.from_numpy(kidx.view(np.int32).copy()).to(dev)
        d_s = torch.from_numpy(sig.copy()).to(dev)
        d_m = torch.from_numpy(blob.copy()).to(dev)
        d_o = torch.from_numpy(off.view(np.int64).copy()).to(dev)
        d_l = torch.from_numpy(ln.view(np.int32).copy()).to(dev)
        stream = torch.cuda.Stream(device=dev)
        for n in args.sizes:
            cpu_t, exp = [], None
            for _ in range(3):
                t, exp = cpu.verify(cache, kidx, sig, blob, off, ln, n, args.threads)
                cpu_t.append(t)
            assert exp.sum() == n - len(bad[bad < n]), "OpenSSL rejects exactly the damaged signatures"
            _, exp_k1 = cpu_k1.verify(cache_k1, kidx, sig_k1, blob, off, ln, n, args.threads)
            nw = (n + 63) // 64
            d_v = torch.zeros(nw, dtype=torch.int64, device=dev)
            ctx.set_profiling(True)
            wall, kern = [], []
            for it in range(2 + args.runs):
                d_v.fill_(-1)
                stream.synchronize()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.ecdsa_verify_device(tid, d_k, d_s, d_m, d_o, d_l, n, d_v, stream)
                stream.synchronize()
                dt = time.perf_counter() - t0
                got = words_to_bools(d_v.cpu().numpy(), n)
                assert np.array_equal(got, exp), f"device-resident verdicts differ at n={n}"
                if it >= 2:
                    wall.append(dt)
                    kern.append(ctx.ecdsa_kernel_ms() * 1e-3)
            ctx.set_profiling(False)
            bitmap = np.zeros((n + 7) // 8, np.uint8)
            hostt, hostt_k1 = [], []
            for it in range(2 + 5):
                dt = host_call(ctx, tid, kidx, sig, blob, off, ln, n, bitmap)
                assert np.array_equal(cb.bitmap_to_bools(bitmap.tobytes(), n), exp), f"host-array verdicts differ at n={n}"
                dk = host_call(ctx, tid_k1, kidx, sig_k1, blob, off, ln, n, bitmap)
                assert np.array_equal(cb.bitmap_to_bools(bitmap.tobytes(), n), exp_k1), f"secp256k1 verdicts differ at n={n}"
                if it >= 2:
                    hostt.append(dt)
                    hostt_k1.append(dk)
            k = median(kern)
            row = {
                "n": n,
                "cpu_openssl_p256_verifies_per_s": n / median(cpu_t),
                "device_resident": {"wall_ms": median(wall) * 1e3, "verifies_per_s": n / median(wall),
                                    "kernel_ms": k * 1e3, "kernel_verifies_per_s": n / k,
                                    "mad64_fraction_of_peak": MAD64_PER_VERIFY * n / k / MAD64_PEAK},
                "host_arrays": {"wall_ms": median(hostt) * 1e3, "verifies_per_s": n / median(hostt)},
                "secp256k1_host_arrays": {"wall_ms": median(hostt_k1) * 1e3, "verifies_per_s": n / median(hostt_k1)},
                "runs": {"device": len(wall), "host_arrays": len(hostt), "cpu": len(cpu_t)},
            }
            row["gpu_over_cpu_device_resident"] = row["device_resident"]["verifies_per_s"] / row["cpu_openssl_p256_verifies_per_s"]
            row["gpu_over_cpu_host_arrays"] = row["host_arrays"]["verifies_per_s"] / row["cpu_openssl_p256_verifies_per_s"]
            result["sizes"].append(row)
            print(json.dumps(row), flush=True)

        # one host-array call against a one-thread OpenSSL P-256 loop
        rows = []

        def sweep(ns):
            for n in ns:
                bitmap = np.zeros((n + 7) // 8, np.uint8)
                g, c = [], []
                for it in range(6):
                    dt = host_call(ctx, tid, kidx, sig, blob, off, ln, n, bitmap)
                    if it:
                        g.append(dt)
                for _ in range(5):
                    t, v = cpu.verify(cache, kidx, sig, blob, off, ln, n, 1)
                    c.append(t)
                assert np.array_equal(cb.bitmap_to_bools(bitmap.tobytes(), n), v)
                rows.append({"n": n, "gpu_call_us": median(g) * 1e6, "host_loop_us": median(c) * 1e6})

        def crossover():
            cross = None
            for r in reversed(rows):
                if r["gpu_call_us"] < r["host_loop_us"]:
                    cross = r["n"]
                else:
                    break
            return cross

        sweep([1 << i for i in range(13)])
        if crossover() is None:
            sweep([8192, 16384])
        cross = crossover()
        result["crossover"] = {"first_n_where_one_call_beats_a_one_thread_loop": cross, "rows": rows}
        ctx.ecdsa_unload_keys(tid)
        ctx.ecdsa_unload_keys(tid_k1)
    cpu.keys_free(cache, NKEYS)
    cpu_k1.keys_free(cache_k1, NKEYS)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"crossover": cross, "out": args.out}))


if __name__ == "__main__":
    main()
