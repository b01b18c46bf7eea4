#!/usr/bin/env python3
"""Throughput of batched RSA-2048 signing (cbft_rsa_sign_batch / _sign_fixed_device) against host
OpenSSL, and the batch size from which the GPU call beats a host sign() loop.

Legs (one signer each; every GPU signature of every leg is compared with OpenSSL's):
  device   65,536 x 32 B, messages and signatures device-resident, for an e = 17 and an e = 65537
           signer (the fault check's cost depends on e); HIP events around `--steps` back-to-back
           calls after `--warmup` calls
  host     the same through host arrays; the call blocks until the signatures are back, so it is
           timed with the host clock around it
  sweep    n = 1 ... 4,096 x 32 B through host arrays against n x the host's per-signature
           EVP_DigestSign time on one core: the crossover (rounded up to a power of two)
  openssl  EVP_DigestSign on 16 threads on the same messages, in the same run
Also reports the multiply-add rate of the schedule actually built against the measured
v_mad_u64_u32 rate of the device (profiles/r01_intrate_microbench.txt).
Writes profiles/rsa_sign.json (or --out) and prints it.
"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("concord-bft_amd", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import cbft_hipcrypto as cb  # noqa: E402
import rsagen  # noqa: E402
from sign_bench import Hip, _p, make_batch  # noqa: E402

MAD_RATE = 3.28e13  # v_mad_u64_u32 multiply-adds per second, whole device (r01 microbenchmark)
# schedule of csrc/rsa_sign.h: 1,300 Montgomery products of 2 x 37 x 37 multiply-adds per lane, two
# lanes, and the 37 x 37 recombination product; the check is the verify kernel's 74-limb products
# (2 x 74 x 74 each): conversion in, one per exponent bit below the top, one per set bit below the
# top, conversion out
SIGN_MACS = 2 * 1300 * 2 * 37 * 37 + 37 * 37


def check_macs(e: int) -> int:
    return (2 + (e.bit_length() - 1) + (bin(e).count("1") - 1)) * 2 * 74 * 74


def _der_len(n):
    if n < 0x80:
        return bytes([n])
    b = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([0x80 | len(b)]) + b


def _der_int(v):
    b = v.to_bytes(v.bit_length() // 8 + 1, "big")
    return b"\x02" + _der_len(len(b)) + b


def crt_params(key):
    p, q, d = key["p"], key["q"], key["d"]
    return (p, q, d % (p - 1), d % (q - 1), pow(q, -1, p), key["e"])


class OpenSSLRsa:
    """EVP_DigestSign (RSA, SHA-256) of the host libcrypto; one EVP_PKEY per worker thread."""

    def __init__(self, key):
        L = self.lib = ctypes.CDLL("libcrypto.so.3")
        L.d2i_AutoPrivateKey.restype = ctypes.c_void_p
        L.d2i_AutoPrivateKey.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_long]
        L.EVP_MD_CTX_new.restype = ctypes.c_void_p
        L.EVP_MD_CTX_free.argtypes = [ctypes.c_void_p]
        L.EVP_sha256.restype = ctypes.c_void_p
        L.EVP_DigestSignInit.argtypes = [ctypes.c_void_p] * 5
        L.EVP_DigestSign.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t),
                                     ctypes.c_void_p, ctypes.c_size_t]
        p, q, dP, dQ, qInv, e = crt_params(key)
        body = b"".join(_der_int(v) for v in (0, key["n"], e, key["d"], p, q, dP, dQ, qInv))
        self.der = b"\x30" + _der_len(len(body)) + body
        self.md = L.EVP_sha256()

    def _pkey(self):
        ptr = ctypes.c_char_p(self.der)
        k = self.lib.d2i_AutoPrivateKey(None, ctypes.byref(ptr), len(self.der))
        if not k:
            raise RuntimeError("PKCS#1 key rejected")
        return k

    def _range(self, blob, msg_len, lo, hi, out):
        L, k = self.lib, self._pkey()
        n = ctypes.c_size_t()
        base, obase = blob.ctypes.data, out.ctypes.data
        for i in range(lo, hi):
            ctx = L.EVP_MD_CTX_new()
            n.value = 256
            ok = L.EVP_DigestSignInit(ctx, None, self.md, None, k) == 1 and \
                L.EVP_DigestSign(ctx, obase + 256 * i, ctypes.byref(n), base + msg_len * i, msg_len) == 1
            L.EVP_MD_CTX_free(ctx)
            if not ok or n.value != 256:
                raise RuntimeError("EVP_DigestSign failed")

    def sign_many(self, blob, msg_len, n, threads):
        """(signatures (n, 256), seconds) over `threads` worker threads (ctypes releases the GIL)."""
        out = np.zeros((n, 256), dtype=np.uint8)
        cuts = [n * t // threads for t in range(threads + 1)]
        t0 = time.perf_counter()
        if threads == 1:
            self._range(blob, msg_len, 0, n, out)
        else:
            with ThreadPoolExecutor(threads) as ex:
                list(ex.map(lambda t: self._range(blob, msg_len, cuts[t], cuts[t + 1], out), range(threads)))
        return out, time.perf_counter() - t0


def sign_host(ctx, tid, blob, off, lens):
    n = int(lens.shape[0])
    out = np.zeros((n, 256), dtype=np.uint8)
    failed = ctypes.c_uint32()
    t0 = time.perf_counter()
    rc = ctx.lib.cbft_rsa_sign_batch(ctx.handle, tid, None, _p(blob), _p(off), _p(lens), n, _p(out),
                                     ctypes.byref(failed))
    dt = time.perf_counter() - t0
    if rc != 0 or failed.value:
        raise cb.CbftError(rc, f"cbft_rsa_sign_batch (failed = {failed.value})")
    return out, dt


def check(sig, exp, what):
    bad = np.nonzero((sig != exp).any(axis=1))[0]
    if bad.size:
        raise SystemExit(f"{what}: {bad.size} of {len(exp)} signatures differ from OpenSSL, first {bad[:8]}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rsa_sign.json"))
    ap.add_argument("--label", default="builder run", help="who ran it (recorded in the JSON)")
    a = ap.parse_args()

    hip = Hip()
    keys = rsagen.load_keys()
    res = {"label": a.label, "n": a.n, "steps": a.steps, "warmup": a.warmup, "threads": a.threads,
           "mad_rate_per_s": MAD_RATE, "sign_macs_per_signature": SIGN_MACS, "legs": {}}
    with cb.Context(device=0, max_batch=a.n) as ctx:
        stream = hip.stream()
        e0, e1 = hip.event(), hip.event()
        blob, off, lens = make_batch(a.n, 32, 1032)
        for ki in (1, 0):  # e = 17 (p > q), e = 65537 (p < q)
            key = keys[ki]
            ossl = OpenSSLRsa(key)
            tid = ctx.rsa_load_signers([crt_params(key)])
            exp, cpu_s = ossl.sign_many(blob, 32, a.n, a.threads)
            d_msg, d_sig = hip.to_dev(blob), hip.malloc(a.n * 256)
            for _ in range(a.warmup):
                ctx.rsa_sign_fixed_device(tid, 0, d_msg, 32, a.n, d_sig, stream)
            hip.record(e0, stream)
            for _ in range(a.steps):
                ctx.rsa_sign_fixed_device(tid, 0, d_msg, 32, a.n, d_sig, stream)
            hip.record(e1, stream)
            dev_ms = hip.elapsed_ms(e0, e1) / a.steps
            check(hip.from_dev(d_sig, a.n * 256).reshape(a.n, 256), exp, f"device e = {key['e']}")
            hip.free(d_msg)
            hip.free(d_sig)
            times = []
            for i in range(a.warmup + a.steps):
                sig, dt = sign_host(ctx, tid, blob, off, lens)
                if i >= a.warmup:
                    times.append(dt)
            check(sig, exp, f"host arrays e = {key['e']}")
            host_ms = 1e3 * float(np.median(times))
            macs = SIGN_MACS + check_macs(key["e"])
            res["legs"][f"{a.n}x32_e{key['e']}"] = {
                "device_ms_per_batch": dev_ms, "device_sigs_per_s": a.n / (dev_ms * 1e-3),
                "host_arrays_ms_per_batch": host_ms, "host_arrays_sigs_per_s": a.n / (host_ms * 1e-3),
                "openssl_threads": a.threads, "openssl_ms_per_batch": 1e3 * cpu_s, "openssl_sigs_per_s": a.n / cpu_s,
                "device_vs_openssl": (a.n / (dev_ms * 1e-3)) / (a.n / cpu_s),
                "host_arrays_vs_openssl": (a.n / (host_ms * 1e-3)) / (a.n / cpu_s),
                "check_macs_per_signature": check_macs(key["e"]),
                "fraction_of_mad_rate": macs * a.n / (dev_ms * 1e-3) / MAD_RATE,
                "all_signatures_equal_openssl": True,
            }
            if ki == 1:
                # crossover sweep under the e = 17 replica key; host sign on one core over 512 signatures
                _, t1 = ossl.sign_many(blob, 32, 512, 1)
                _, t1b = ossl.sign_many(blob, 32, 512, 1)
                host_sign_us = 1e6 * min(t1, t1b) / 512
                sweep, crossover = [], None
                for n in (1, 2, 4, 8, 16, 32, 64, 128, 256, 1024, 4096):
                    b, o, ln = blob[: n * 32], off[:n], lens[:n]
                    times = []
                    for i in range(2 + 5):
                        sig, dt = sign_host(ctx, tid, b, o, ln)
                        if i >= 2:
                            times.append(dt)
                    check(sig, exp[:n], f"sweep n = {n}")
                    gpu_us = 1e6 * float(np.median(times))
                    wins = gpu_us < n * host_sign_us
                    sweep.append({"n": n, "gpu_call_us": gpu_us, "host_loop_us": n * host_sign_us,
                                  "gpu_wins": bool(wins)})
                    if not wins:
                        crossover = None  # the crossover is the size from which the GPU wins at every larger one
                    elif crossover is None:
                        crossover = n
                res["host_sign_us_one_core"] = host_sign_us
                res["sweep"] = sweep
                res["crossover_n"] = crossover
                res["crossover_pow2"] = None if crossover is None else 1 << (crossover - 1).bit_length()
            ctx.rsa_unload_signers(tid)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
