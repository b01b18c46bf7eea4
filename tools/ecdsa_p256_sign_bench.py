#!/usr/bin/env python3
"""Throughput of batched ECDSA P-256 signing (cbft_ecdsa_sign_batch / _sign_fixed_device on a
CBFT_CURVE_P256 signer table) against host OpenSSL threads, against cbft_ecdsa_verify_batch on a P-256
key table at the same size, and against the secp256k1 signer at the same size in the same run; and the
batch size from which one GPU call beats a loop of the host build of the lane code on one core.

Legs (one signer; every timed batch is checked: all signatures accepted by OpenSSL on 16 threads and by
cbft_ecdsa_verify_batch on a P-256 table, all equal to the host build's, 256 sampled ones equal to
tests/p256_sign_ref.py):
  device   65,536 x 32 B, 65,536 x 256 B, 4,096 x 32 B, 262,144 x 32 B, messages and signatures
           device-resident; events around `--steps` back-to-back calls after `--warmup` calls
  host     the same shapes through host arrays (the call blocks; host clock around it)
  kernel   cbft_ecdsa_sign_kernel_ms of one profiled batch; the verify kernels' time on the same
           signatures (cbft_ecdsa_kernel_ms)
  k1       the secp256k1 signer on the same messages: device-resident time and kernel time
  openssl  ecdsa_p256_sign_many of tools/cpu_baseline/openssl_ecdsa_p256_sign.c (SHA256 + ECDSA_do_sign,
           cached EC_KEYs) on 16 threads, same run
  sweep    n = 1 .. 1,024 x 32 B through host arrays against a timed loop of the host lane code over
           the same n messages on one core (the crossover, rounded up to a power of two), with a
           one-thread OpenSSL ECDSA_do_sign loop over the same messages beside it
Writes profiles/ecdsa_p256_sign.json (or --out) and prints it.
"""
import argparse
import ctypes
import json
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("concord-bft_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import cbft_hipcrypto as cb  # noqa: E402
import p256_sign_ref as sref  # noqa: E402

VP = ctypes.c_void_p
SHAPES = ((65536, 32), (65536, 256), (4096, 32), (262144, 32))


def _p(a):
    return a.ctypes.data_as(VP)


def median(xs):
    return float(np.median(np.asarray(xs, dtype=np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecdsa_p256_sign.json"))
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    cpu = ctypes.CDLL(os.path.join(ROOT, "tools", "cpu_baseline", "libcbft_cpu_openssl_ecdsa_p256.so"))
    cpu.cbft_cpu_p256_keys_new.restype = VP
    cpu_sign = ctypes.CDLL(os.path.join(ROOT, "tools", "cpu_baseline", "libcbft_cpu_openssl_ecdsa_p256_sign.so"))
    cpu_sign.ecdsa_p256_sign_keys_new.restype = VP
    shim = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libecdsa_p256_sign_shim.so"))
    rng = np.random.default_rng(0xEC5C)
    x = int.from_bytes(rng.bytes(32), "big") % (sref.N - 1) + 1
    priv = np.frombuffer(x.to_bytes(32, "big"), dtype=np.uint8).copy()
    pub = np.frombuffer(sref.public_key(x), dtype=np.uint8).copy()
    zero_idx = np.zeros(max(n for n, _ in SHAPES), dtype=np.uint32)
    cache = VP(cpu.cbft_cpu_p256_keys_new(_p(pub), 1))
    sign_cache = VP(cpu_sign.ecdsa_p256_sign_keys_new(_p(priv), 1))
    assert cache and sign_cache

    torch.zeros(1, device="cuda:0")
    dev = torch.device("cuda:0")
    result = {
        "what": "ECDSA P-256 / SHA-256 batch signing (RFC 6979), one GPU against host OpenSSL threads, one run",
        "box": {"gpu": torch.cuda.get_device_name(0), "host_cpu": platform.processor() or platform.machine()},
        "cpu_threads": args.threads, "steps": args.steps, "warmup": args.warmup, "sizes": [],
    }

    def host_lane(blob, L, n, threads):
        out = np.zeros((n, 64), dtype=np.uint8)
        t0 = time.perf_counter()
        shim.ecdsa_p256_sign_shim_sign_many(_p(priv), None, _p(blob), ctypes.c_uint32(L), ctypes.c_size_t(n), _p(out),
                                            ctypes.c_int(threads))
        return time.perf_counter() - t0, out

    def openssl_sign(blob, off, ln, n, threads):
        out = np.zeros(n * 64, np.uint8)
        t0 = time.perf_counter()
        assert cpu_sign.ecdsa_p256_sign_many(sign_cache, None, _p(blob), _p(off), _p(ln), ctypes.c_size_t(n), _p(out),
                                             threads) == 0
        return time.perf_counter() - t0

    with cb.Context(0) as ctx:
        tid = ctx.ecdsa_load_signers(priv.reshape(1, 32), curve="p256")
        k1_tid = ctx.ecdsa_load_signers(priv.reshape(1, 32))  # the same scalar is a secp256k1 key too
        vt = ctx.ecdsa_load_keys(pub.reshape(1, 64), curve="p256")
        stream = torch.cuda.Stream(device=dev)

        def host_call(table, blob, off, ln, n, out):
            t0 = time.perf_counter()
            rc = ctx.lib.cbft_ecdsa_sign_batch(ctx.handle, table, None, _p(blob), _p(off), _p(ln), ctypes.c_size_t(n), _p(out))
            assert rc == 0, rc
            return time.perf_counter() - t0

        def device_leg(table, d_m, L, n, d_s):
            for _ in range(args.warmup):
                ctx.ecdsa_sign_device(table, None, d_m, L, n, d_s, stream)
            stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                ctx.ecdsa_sign_device(table, None, d_m, L, n, d_s, stream)
            e1.record(stream)
            stream.synchronize()
            return e0.elapsed_time(e1) / 1e3 / args.steps

        for n, L in SHAPES:
            blob = rng.integers(0, 256, n * L, dtype=np.uint8)
            off = np.arange(n, dtype=np.uint64) * np.uint64(L)
            ln = np.full(n, L, dtype=np.uint32)
            ossl = [openssl_sign(blob, off, ln, n, args.threads) for _ in range(3)]
            d_m = torch.from_numpy(blob.copy()).to(dev)
            d_s = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
            d_k1 = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
            k1_dev_s = device_leg(k1_tid, d_m, L, n, d_k1)
            dev_s = device_leg(tid, d_m, L, n, d_s)
            got = d_s.cpu().numpy().reshape(n, 64)
            hout = np.zeros((n, 64), dtype=np.uint8)
            host_t = [host_call(tid, blob, off, ln, n, hout) for _ in range(3)]
            # one profiled batch of each signer; the verify kernels on the same signatures
            ctx.set_profiling(True)
            k1out = np.zeros((n, 64), dtype=np.uint8)
            host_call(k1_tid, blob, off, ln, n, k1out)
            k1_kernel_ms = ctx.ecdsa_sign_kernel_ms()
            host_call(tid, blob, off, ln, n, hout)
            kernel_ms = ctx.ecdsa_sign_kernel_ms()
            d_v = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
            d_k = torch.zeros(n, dtype=torch.int32, device=dev)
            d_o = torch.from_numpy(off.view(np.int64).copy()).to(dev)
            d_l = torch.from_numpy(ln.view(np.int32).copy()).to(dev)
            ctx.ecdsa_verify_device(vt, d_k, d_s, d_m, d_o, d_l, n, d_v, stream)
            stream.synchronize()
            verify_ms = ctx.ecdsa_kernel_ms()
            ctx.set_profiling(False)
            accepted_gpu = int(np.unpackbits(d_v.cpu().numpy().view(np.uint8), bitorder="little")[:n].sum())
            # checks on the timed batch
            _, lane = host_lane(blob, L, n, args.threads)
            ok = np.zeros(n, np.uint8)
            cpu.cbft_cpu_p256_verify(cache, _p(zero_idx), _p(got), _p(blob), _p(off), _p(ln), ctypes.c_size_t(n), _p(ok),
                                     args.threads)
            sample = rng.choice(n, size=256, replace=False)
            ref_ok = all(got[i].tobytes() == sref.sign(x, blob[i * L:(i + 1) * L].tobytes()) for i in sample)
            checks = {"openssl_accepts": int(ok.sum()), "equal_host_build": int((got == lane).all(axis=1).sum()),
                      "host_array_equal_device": bool(np.array_equal(hout, got)), "sample_256_equal_restatement": ref_ok,
                      "gpu_verify_accepts": accepted_gpu}
            assert checks["openssl_accepts"] == n and checks["equal_host_build"] == n and ref_ok, checks
            assert checks["host_array_equal_device"] and accepted_gpu == n, checks
            row = {"n": n, "msg_len": L,
                   "device_resident_sigs_per_s": n / dev_s, "device_resident_ms": dev_s * 1e3,
                   "host_array_sigs_per_s": n / median(host_t), "host_array_ms": median(host_t) * 1e3,
                   "sign_kernel_ms": kernel_ms, "verify_kernels_ms_same_n": verify_ms,
                   "sign_over_verify_kernel_time": kernel_ms / verify_ms,
                   "secp256k1_device_resident_ms": k1_dev_s * 1e3, "secp256k1_sign_kernel_ms": k1_kernel_ms,
                   "p256_over_secp256k1_device_time": dev_s / k1_dev_s,
                   "openssl_threads_sigs_per_s": n / min(ossl),
                   "device_over_openssl_threads": (n / dev_s) / (n / min(ossl)), "checks": checks}
            result["sizes"].append(row)
            print(json.dumps(row), flush=True)

        # crossover against a loop of the host lane code on one core; OpenSSL on one thread beside it
        L = 32
        blob = rng.integers(0, 256, 1024 * L, dtype=np.uint8)
        off = np.arange(1024, dtype=np.uint64) * np.uint64(L)
        ln = np.full(1024, L, dtype=np.uint32)
        host_lane(blob, L, 64, 1)  # builds the host comb table outside the timed loops
        sweep, cross = [], None
        hout = np.zeros((1024, 64), dtype=np.uint8)
        n = 1
        while n <= 1024:
            t = median([host_call(tid, blob, off, ln, n, hout) for _ in range(9)])
            th = median([host_lane(blob, L, n, 1)[0] for _ in range(5 if n <= 64 else 3)])
            to = median([openssl_sign(blob, off, ln, n, 1) for _ in range(5 if n <= 64 else 3)])
            sweep.append({"n": n, "gpu_call_us": t * 1e6, "host_loop_us": th * 1e6, "openssl_one_thread_us": to * 1e6})
            if cross is None and t < th:
                cross = n
            n *= 2
        result["crossover"] = {"host_loop": "the host build of the lane code over the same n messages, one thread, timed at each n",
                               "openssl_one_thread": "SHA256 + ECDSA_do_sign on prime256v1 over the same n messages, one thread",
                               "sweep": sweep, "first_n_where_gpu_call_wins": cross}
        ctx.ecdsa_unload_signers(tid)
        ctx.ecdsa_unload_signers(k1_tid)
        ctx.ecdsa_unload_keys(vt)
    cpu.cbft_cpu_p256_keys_free(cache, 1)
    cpu_sign.ecdsa_p256_sign_keys_free(sign_cache, 1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["crossover"]))


if __name__ == "__main__":
    main()
