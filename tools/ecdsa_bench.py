#!/usr/bin/env python3
"""ECDSA secp256k1 / SHA-256 batch verification on one GPU against the host OpenSSL, in one run.

    python3 tools/ecdsa_bench.py [--out profiles/ecdsa_verify.json] [--threads 16]

Sizes: 65,536 and 4,096 signatures over 256-byte messages and 4,096 keys, one in a hundred damaged,
and 262,144 of the same to show what the chip gives once every SIMD holds more than one wave.
Modes: device-resident arrays (cbft_ecdsa_verify_batch_device, wall time to a synchronised stream and
the kernels' own time from cbft_ecdsa_kernel_ms) and host arrays (cbft_ecdsa_verify_batch, copies
included).  The baseline of the same run is `threads` host threads of SHA256 + ECDSA_do_verify with
cached EC_KEYs (tools/cpu_baseline/openssl_ecdsa.c), whose verdicts are also the expected ones: every
GPU verdict of every timed run is compared with them.  Last, the batch size from which one host-array
call beats a one-thread host loop.  Warm runs first, then medians; the box is named in the output.

MAD64 fraction: executed v_mad_u64_u32 per verification x n / kernel time / 39.32e12.  The count is
74 per field multiplication (the ISA listing of fe_mul, hipcc -S --cuda-device-only, gfx950) times
the multiplications a verification with random scalars runs: 64 windows x (4 doublings x 7 + 2 x
15/16 mixed additions x 11) + 3 for the closing comparison, plus 2 x 224 for the two products mod n.
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

CPU_SO = os.path.join(ROOT, "tools", "cpu_baseline", "libcbft_cpu_openssl_ecdsa.so")
MAD64_PEAK = 39.32e12
MAD64_PER_FE_MUL = 74
FE_MUL_PER_VERIFY = 64 * (4 * 7 + 2 * 15 / 16 * 11) + 3
MAD64_PER_VERIFY = MAD64_PER_FE_MUL * FE_MUL_PER_VERIFY + 2 * 224
NKEYS = 4096
MSG_LEN = 256


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Cpu:
    def __init__(self):
        self.lib = ctypes.CDLL(CPU_SO)
        self.lib.cbft_cpu_ecdsa_keys_new.restype = ctypes.c_void_p
        self.lib.cbft_cpu_ecdsa_keys_new.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        self.lib.cbft_cpu_ecdsa_keys_free.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        self.lib.cbft_cpu_ecdsa_verify.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
        self.lib.cbft_cpu_ecdsa_keygen.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        self.lib.cbft_cpu_ecdsa_sign_many.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4 + [
            ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]

    def keygen(self, nkeys):
        priv, pub = np.zeros(nkeys * 32, np.uint8), np.zeros(nkeys * 64, np.uint8)
        assert self.lib.cbft_cpu_ecdsa_keygen(nkeys, _p(priv), _p(pub)) == 0
        return priv, pub

    def sign(self, priv, nkeys, kidx, blob, off, ln, threads):
        sig = np.zeros(len(kidx) * 64, np.uint8)
        assert self.lib.cbft_cpu_ecdsa_sign_many(_p(priv), nkeys, _p(kidx), _p(blob), _p(off), _p(ln), len(kidx), _p(sig),
                                                 threads) == 0
        return sig

    def verify(self, cache, kidx, sig, blob, off, ln, n, threads):
        out = np.zeros(n, np.uint8)
        t0 = time.perf_counter()
        self.lib.cbft_cpu_ecdsa_verify(cache, _p(kidx), _p(sig), _p(blob), _p(off), _p(ln), n, _p(out), threads)
        return time.perf_counter() - t0, out.astype(bool)


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def words_to_bools(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecdsa_verify.json"))
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()

    cpu = Cpu()
    rng = np.random.default_rng(0xECD5A)
    nmax = 262144
    priv, pub = cpu.keygen(NKEYS)
    kidx = rng.integers(0, NKEYS, nmax, dtype=np.uint32)
    blob = rng.integers(0, 256, nmax * MSG_LEN, dtype=np.uint8)
    off = (np.arange(nmax, dtype=np.uint64) * MSG_LEN)
    ln = np.full(nmax, MSG_LEN, dtype=np.uint32)
    sig = cpu.sign(priv, NKEYS, kidx, blob, off, ln, args.threads)
    bad = np.arange(37, nmax, 100)
    sig[bad * 64 + (bad % 64)] ^= np.uint8(1) << (bad % 8).astype(np.uint8)  # one bit of r or s
    cache = cpu.lib.cbft_cpu_ecdsa_keys_new(_p(pub), NKEYS)

    torch.zeros(1, device="cuda:0")
    dev = torch.device("cuda:0")
    result = {
        "what": "ECDSA secp256k1 / SHA-256 batch verification, one GPU against host OpenSSL threads, one run",
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
        tid = ctx.ecdsa_load_keys(pub.reshape(-1, 64))
        assert ctx.ecdsa_key_status(tid, NKEYS).all()
        d_k = torch.from_numpy(kidx.view(np.int32).copy()).to(dev)
        d_s = torch.from_numpy(sig.copy()).to(dev)
        d_m = torch.from_numpy(blob.copy()).to(dev)
        d_o = torch.from_numpy(off.view(np.int64).copy()).to(dev)
        d_l = torch.from_numpy(ln.view(np.int32).copy()).to(dev)
        stream = torch.cuda.Stream(device=dev)
        for n in (65536, 4096, 262144):
            cpu_t, exp = [], None
            for _ in range(3):
                t, v = cpu.verify(cache, kidx, sig, blob, off, ln, n, args.threads)
                cpu_t.append(t)
                exp = v
            assert exp.sum() == n - len(bad[bad < n]), "OpenSSL rejects exactly the damaged signatures"
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
            hostt = []
            bitmap = np.zeros((n + 7) // 8, np.uint8)
            for it in range(1 + 5):
                bitmap[:] = 0xFF
                t0 = time.perf_counter()
                rc = ctx.lib.cbft_ecdsa_verify_batch(ctx.handle, tid, _p(kidx), _p(sig), _p(blob), _p(off), _p(ln), n,
                                                     _p(bitmap))
                dt = time.perf_counter() - t0
                assert rc == 0
                assert np.array_equal(cb.bitmap_to_bools(bitmap.tobytes(), n), exp), f"host-array verdicts differ at n={n}"
                if it >= 1:
                    hostt.append(dt)
            k = median(kern)
            row = {
                "n": n,
                "cpu_openssl_verifies_per_s": n / median(cpu_t),
                "device_resident": {"wall_ms": median(wall) * 1e3, "verifies_per_s": n / median(wall),
                                    "kernel_ms": k * 1e3, "kernel_verifies_per_s": n / k,
                                    "mad64_fraction_of_peak": MAD64_PER_VERIFY * n / k / MAD64_PEAK},
                "host_arrays": {"wall_ms": median(hostt) * 1e3, "verifies_per_s": n / median(hostt)},
                "runs": {"device": len(wall), "host_arrays": len(hostt), "cpu": len(cpu_t)},
            }
            row["gpu_over_cpu_device_resident"] = row["device_resident"]["verifies_per_s"] / row["cpu_openssl_verifies_per_s"]
            result["sizes"].append(row)
            print(json.dumps(row), flush=True)

        # one host-array call against a one-thread host loop
        cross, rows = None, []
        for n in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
            bitmap = np.zeros((n + 7) // 8, np.uint8)
            g, c = [], []
            for it in range(6):
                t0 = time.perf_counter()
                rc = ctx.lib.cbft_ecdsa_verify_batch(ctx.handle, tid, _p(kidx), _p(sig), _p(blob), _p(off), _p(ln), n,
                                                     _p(bitmap))
                dt = time.perf_counter() - t0
                assert rc == 0
                if it:
                    g.append(dt)
            for _ in range(5):
                t, v = cpu.verify(cache, kidx, sig, blob, off, ln, n, 1)
                c.append(t)
            assert np.array_equal(cb.bitmap_to_bools(bitmap.tobytes(), n), v)
            rows.append({"n": n, "gpu_call_us": median(g) * 1e6, "host_loop_us": median(c) * 1e6})
        for r in reversed(rows):
            if r["gpu_call_us"] < r["host_loop_us"]:
                cross = r["n"]
            else:
                break
        result["crossover"] = {"first_n_where_one_call_beats_a_one_thread_loop": cross, "rows": rows}
        ctx.ecdsa_unload_keys(tid)
    cpu.lib.cbft_cpu_ecdsa_keys_free(cache, NKEYS)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"crossover": cross, "out": args.out}))


if __name__ == "__main__":
    main()
