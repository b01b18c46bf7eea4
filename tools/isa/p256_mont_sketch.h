// The rejected Montgomery form of the P-256 field reduction, kept for its instruction
// count (tools/isa/p256_fe_mul_probe.hip, `make p256_isa`) and checked on the host against Python integers by
// tests/test_ecdsa_p256_cpu.py through the shim.  x[0..16) -> x / 2^256 mod p, canonical.
#pragma once
#include "fe_p256.h"

// Montgomery reduction for p = 2^256 - 2^224 + 2^192 + 2^96 - 1 (p = -1 mod 2^32: m = the low word)
K1_HD void mont_reduce512(P2Fe& r, const uint32_t* x) {
  int64_t col[17];
#pragma unroll
  for (int i = 0; i < 16; i++) col[i] = x[i];
  col[16] = 0;
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += col[i];
    const int64_t m = (uint32_t)c;
    c = (c - m) >> 32;
    col[i + 3] += m;
    col[i + 6] += m;
    col[i + 7] -= m;
    col[i + 8] += m;
  }
  uint32_t t[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += col[8 + i];
    t[i] = (uint32_t)c;
    c >>= 32;
  }
  c += col[16];  // the carry out: small and signed
  c = p2_fold(t, c);
  (void)p2_fold(t, c);
  p2_fe_final(r, t, 0);
}
