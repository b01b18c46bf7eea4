#!/usr/bin/env python3
"""Throughput of batched Ed25519 signing (cbft_ed25519_sign_batch / _sign_fixed_device) against
host OpenSSL, and the batch size from which the GPU call beats a host sign() loop.

Legs (all with one signer; every GPU signature of every leg is compared with OpenSSL's and
verified with cbft_ed25519_verify_batch):
  device   65,536 x 32 B and x 256 B, messages and signatures device-resident; HIP events around
           `--steps` back-to-back calls after `--warmup` calls
  host     the same shapes through host arrays; the call blocks until the signatures are back, so
           it is timed with the host clock around it
  sweep    n = 1, 16, 64, 256, 1K, 4K x 32 B through host arrays against n x the host's
           per-signature sign() time on one core: the crossover (rounded up to a power of two)
  openssl  cbft_cpu_sign_many on 16 threads on the same messages, in the same run
Writes profiles/ed25519_sign.json (or --out) and prints it.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("concord-bft_amd", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))
import cbft_hipcrypto as cb  # noqa: E402
import workload  # noqa: E402

VP = ctypes.c_void_p


def _p(a):
    return a.ctypes.data_as(VP)


class Hip:
    def __init__(self):
        cb.load_library()
        self.lib = ctypes.CDLL("libamdhip64.so.7")  # the runtime libcbft_hipcrypto linked
        self.lib.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), VP, VP]

    def ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: hipError {rc}")

    def malloc(self, nbytes):
        p = VP()
        self.ok(self.lib.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(nbytes, 1))), "hipMalloc")
        return p.value

    def to_dev(self, a):
        a = np.ascontiguousarray(a)
        p = self.malloc(a.nbytes)
        self.ok(self.lib.hipMemcpy(VP(p), _p(a), ctypes.c_size_t(a.nbytes), 1), "hipMemcpy H2D")
        return p

    def from_dev(self, ptr, nbytes):
        out = np.zeros(nbytes, dtype=np.uint8)
        self.ok(self.lib.hipMemcpy(_p(out), VP(ptr), ctypes.c_size_t(nbytes), 2), "hipMemcpy D2H")
        return out

    def free(self, ptr):
        self.lib.hipFree(VP(ptr))

    def stream(self):
        s = VP()
        self.ok(self.lib.hipStreamCreate(ctypes.byref(s)), "hipStreamCreate")
        return s.value

    def event(self):
        e = VP()
        self.ok(self.lib.hipEventCreate(ctypes.byref(e)), "hipEventCreate")
        return e.value

    def record(self, e, s):
        self.ok(self.lib.hipEventRecord(VP(e), VP(s)), "hipEventRecord")

    def elapsed_ms(self, a, b):
        self.ok(self.lib.hipEventSynchronize(VP(b)), "hipEventSynchronize")
        ms = ctypes.c_float()
        self.ok(self.lib.hipEventElapsedTime(ctypes.byref(ms), VP(a), VP(b)), "hipEventElapsedTime")
        return ms.value


def make_batch(n, msg_len, seed):
    rng = np.random.default_rng(seed)
    blob = rng.integers(0, 256, size=n * msg_len, dtype=np.uint8)
    off = np.arange(n, dtype=np.uint64) * np.uint64(msg_len)
    lens = np.full(n, msg_len, dtype=np.uint32)
    return blob, off, lens


def openssl_sign(seed32, blob, off, lens, threads):
    """(signatures, seconds) of cbft_cpu_sign_many."""
    n = int(lens.shape[0])
    sig = np.zeros((n, 64), dtype=np.uint8)
    idx = np.zeros(n, dtype=np.uint32)
    lib = workload.cpu_lib()
    t0 = time.perf_counter()
    lib.cbft_cpu_sign_many(_p(seed32), 1, _p(idx), _p(blob), _p(off), _p(lens), n, _p(sig), threads)
    return sig, time.perf_counter() - t0


def sign_host(ctx, tid, blob, off, lens):
    n = int(lens.shape[0])
    out = np.zeros((n, 64), dtype=np.uint8)
    t0 = time.perf_counter()
    rc = ctx.lib.cbft_ed25519_sign_batch(ctx.handle, tid, None, _p(blob), _p(off), _p(lens), n, _p(out))
    dt = time.perf_counter() - t0
    if rc != 0:
        raise cb.CbftError(rc, "cbft_ed25519_sign_batch")
    return out, dt


def check(ctx, vt, sig, exp, blob, off, lens, what):
    """Every signature equals OpenSSL's and verifies on the GPU."""
    n = int(lens.shape[0])
    bad = np.nonzero((sig != exp).any(axis=1))[0]
    if bad.size:
        raise SystemExit(f"{what}: {bad.size} of {n} signatures differ from OpenSSL, first {bad[:8]}")
    ok = cb.bitmap_to_bools(ctx.verify_packed(vt, np.zeros(n, dtype=np.uint32), sig, blob, off, lens), n)
    if not ok.all():
        raise SystemExit(f"{what}: {int((~ok).sum())} signatures do not verify")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ed25519_sign.json"))
    ap.add_argument("--label", default="builder run", help="who ran it (recorded in the JSON)")
    a = ap.parse_args()

    hip = Hip()
    seed32 = np.frombuffer(bytes(range(7, 39)), dtype=np.uint8).copy()
    res = {"label": a.label, "n": a.n, "steps": a.steps, "warmup": a.warmup, "threads": a.threads, "legs": {}}
    with cb.Context(device=0, max_batch=a.n) as ctx:
        tid = ctx.load_signers(seed32.reshape(1, 32))
        vt = ctx.load_keys(ctx.signer_public_keys(tid))
        stream = hip.stream()
        e0, e1 = hip.event(), hip.event()
        for msg_len in (32, 256):
            blob, off, lens = make_batch(a.n, msg_len, 1000 + msg_len)
            exp, cpu_s = openssl_sign(seed32, blob, off, lens, a.threads)
            _, cpu_s2 = openssl_sign(seed32, blob, off, lens, a.threads)  # second pass: warm
            cpu_s = min(cpu_s, cpu_s2)
            # device-resident
            d_msg, d_sig = hip.to_dev(blob), hip.malloc(a.n * 64)
            for _ in range(a.warmup):
                ctx.sign_fixed_device(tid, 0, d_msg, msg_len, a.n, d_sig, stream)
            hip.record(e0, stream)
            for _ in range(a.steps):
                ctx.sign_fixed_device(tid, 0, d_msg, msg_len, a.n, d_sig, stream)
            hip.record(e1, stream)
            dev_ms = hip.elapsed_ms(e0, e1) / a.steps
            check(ctx, vt, hip.from_dev(d_sig, a.n * 64).reshape(a.n, 64), exp, blob, off, lens,
                  f"device {a.n} x {msg_len}")
            hip.free(d_msg)
            hip.free(d_sig)
            # host arrays
            times = []
            for i in range(a.warmup + a.steps):
                sig, dt = sign_host(ctx, tid, blob, off, lens)
                if i >= a.warmup:
                    times.append(dt)
            check(ctx, vt, sig, exp, blob, off, lens, f"host {a.n} x {msg_len}")
            host_ms = 1e3 * float(np.median(times))
            res["legs"][f"{a.n}x{msg_len}"] = {
                "device_ms_per_batch": dev_ms, "device_sigs_per_s": a.n / (dev_ms * 1e-3),
                "host_arrays_ms_per_batch": host_ms, "host_arrays_sigs_per_s": a.n / (host_ms * 1e-3),
                "openssl_threads": a.threads, "openssl_ms_per_batch": 1e3 * cpu_s, "openssl_sigs_per_s": a.n / cpu_s,
                "device_vs_openssl": (a.n / (dev_ms * 1e-3)) / (a.n / cpu_s),
                "host_arrays_vs_openssl": (a.n / (host_ms * 1e-3)) / (a.n / cpu_s),
                "all_signatures_equal_openssl_and_verify": True,
            }
        # crossover sweep, 32-byte messages; host sign() on one core measured over 4,096 signatures
        blob, off, lens = make_batch(4096, 32, 77)
        exp, t1 = openssl_sign(seed32, blob, off, lens, 1)
        _, t1b = openssl_sign(seed32, blob, off, lens, 1)
        host_sign_us = 1e6 * min(t1, t1b) / 4096
        sweep, crossover = [], None
        for n in (1, 16, 64, 256, 1024, 4096):
            b, o, ln = blob[: n * 32], off[:n], lens[:n]
            times = []
            for i in range(3 + 9):
                sig, dt = sign_host(ctx, tid, b, o, ln)
                if i >= 3:
                    times.append(dt)
            check(ctx, vt, sig, exp[:n], b, o, ln, f"sweep n = {n}")
            gpu_us = 1e6 * float(np.median(times))
            wins = gpu_us < n * host_sign_us
            sweep.append({"n": n, "gpu_call_us": gpu_us, "host_loop_us": n * host_sign_us, "gpu_wins": bool(wins)})
            if wins and crossover is None:
                crossover = n
        res["host_sign_us_one_core"] = host_sign_us
        res["sweep"] = sweep
        res["crossover_n"] = crossover
        res["crossover_pow2"] = None if crossover is None else 1 << (crossover - 1).bit_length()
        ctx.unload_keys(vt)
        ctx.unload_signers(tid)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
