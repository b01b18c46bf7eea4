// GF(p), p = 2^256 - 2^32 - 977 (secp256k1), for ECDSA verification: everything here works on
// PUBLIC values and may branch on them.  Eight little-endian 32-bit limbs, always canonical
// (in [0, p)), products on the INT32 VALU (each a[i] * b[j] + r + carry step is one
// v_mad_u64_u32), reduction with 2^256 = 2^32 + 977 (mod p).  Host and device from one source.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define K1_HD __host__ __device__ __forceinline__
#else
#define K1_HD inline
#endif
#include "safegcd30.h"

struct K1Fe {
  uint32_t v[8];
};

// ---- 256-bit helpers shared with sc_secp256k1.h ------------------------------------------------
// r = a + b, returns the carry out
K1_HD uint32_t k1_add256(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)a[i] + b[i];
    r[i] = (uint32_t)c;
    c >>= 32;
  }
  return (uint32_t)c;
}
// r = a - b, returns the borrow out (1 when a < b)
K1_HD uint32_t k1_sub256(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (int64_t)a[i] - (int64_t)b[i];
    r[i] = (uint32_t)c;
    c >>= 32;
  }
  return (uint32_t)(c & 1);
}
K1_HD bool k1_is_zero256(const uint32_t* a) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) x |= a[i];
  return x == 0;
}
K1_HD bool k1_eq256(const uint32_t* a, const uint32_t* b) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) x |= a[i] ^ b[i];
  return x == 0;
}
// 32 big-endian bytes -> limbs
K1_HD void k1_from_be(uint32_t* r, const uint8_t* b) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = b + 4 * (7 - i);
    r[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
}
K1_HD void k1_to_be(uint8_t* b, const uint32_t* a) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint8_t* q = b + 4 * (7 - i);
    q[0] = (uint8_t)(a[i] >> 24);
    q[1] = (uint8_t)(a[i] >> 16);
    q[2] = (uint8_t)(a[i] >> 8);
    q[3] = (uint8_t)a[i];
  }
}
// r[0..16) = a * b (operand scanning: a[i] b[j] + r[i + j] + carry < 2^64)
K1_HD void k1_mul512(uint32_t* r, const uint32_t* a, const uint32_t* b) {
#pragma unroll
  for (int i = 0; i < 16; i++) r[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      c += (uint64_t)a[i] * b[j] + r[i + j];
      r[i + j] = (uint32_t)c;
      c >>= 32;
    }
    r[i + 8] = (uint32_t)c;
  }
}
// 8 x 32-bit limbs of a value < 2^256 <-> 9 signed-30 limbs (safegcd30.h)
K1_HD void k1_to_s30(Sg30& x, const uint32_t* a) {
#pragma unroll
  for (int j = 0; j < 9; j++) {
    const int b = 30 * j, i = b / 32, s = b % 32;
    const uint64_t w = ((uint64_t)(i + 1 < 8 ? a[i + 1] : 0u) << 32) | a[i];
    x.v[j] = (int32_t)((w >> s) & SG_M30);
  }
}
K1_HD void k1_from_s30(uint32_t* a, const Sg30& x) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int b = 32 * i, j = b / 30, s = b % 30;
    // limbs j, j + 1 and (when s > 28) j + 2 cover bits [b, b + 32)
    uint64_t w = ((uint64_t)(uint32_t)x.v[j] >> s) | ((uint64_t)(uint32_t)x.v[j + 1] << (30 - s));
    if (j + 2 < 9) w |= (uint64_t)(uint32_t)x.v[j + 2] << (60 - s);
    a[i] = (uint32_t)w;
  }
}

// ---- the field ---------------------------------------------------------------------------------
#define K1_P_LIMBS                                                                                  \
  { 0xFFFFFC2Fu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu }

struct K1FeS30 {  // p in signed-30 limbs, p^-1 mod 2^30
  static constexpr int32_t P[9] = {0x3ffffc2f, 0x3ffffffb, 0x3fffffff, 0x3fffffff, 0x3fffffff,
                                   0x3fffffff, 0x3fffffff, 0x3fffffff, 0x0000ffff};
  static constexpr uint32_t PINV30 = 0x2ddacacfu;
};

K1_HD void fe_zero(K1Fe& r) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = 0;
}
K1_HD void fe_one(K1Fe& r) {
  fe_zero(r);
  r.v[0] = 1;
}
K1_HD bool fe_is_zero(const K1Fe& a) { return k1_is_zero256(a.v); }
K1_HD bool fe_eq(const K1Fe& a, const K1Fe& b) { return k1_eq256(a.v, b.v); }

// t < 2^256 (+ carry 2^256) -> t mod p, given t + carry 2^256 < 2 p
K1_HD void fe_final(K1Fe& r, const uint32_t* t, uint32_t carry) {
  const uint32_t P[8] = K1_P_LIMBS;
  uint32_t u[8];
  const uint32_t borrow = k1_sub256(u, t, P);
  const uint32_t take = (carry | (borrow ^ 1u)) ? 0xFFFFFFFFu : 0u;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (u[i] & take) | (t[i] & ~take);
}
// 32 big-endian bytes -> r; false (r unspecified) unless the value is below p
K1_HD bool fe_from_be(K1Fe& r, const uint8_t* b) {
  const uint32_t P[8] = K1_P_LIMBS;
  uint32_t u[8];
  k1_from_be(r.v, b);
  return k1_sub256(u, r.v, P) != 0;
}
K1_HD void fe_add(K1Fe& r, const K1Fe& a, const K1Fe& b) {
  uint32_t t[8];
  const uint32_t c = k1_add256(t, a.v, b.v);
  fe_final(r, t, c);
}
K1_HD void fe_sub(K1Fe& r, const K1Fe& a, const K1Fe& b) {
  const uint32_t P[8] = K1_P_LIMBS;
  uint32_t t[8];
  const uint32_t m = k1_sub256(t, a.v, b.v) ? 0xFFFFFFFFu : 0u;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)t[i] + (P[i] & m);
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
}
K1_HD void fe_neg(K1Fe& r, const K1Fe& a) {
  K1Fe z;
  fe_zero(z);
  fe_sub(r, z, a);
}
// x[0..16) -> x mod p
K1_HD void fe_reduce512(K1Fe& r, const uint32_t* x) {
  // fold 1: t = lo + hi * 977 + (hi << 32) < 2^289
  uint32_t t[10];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)x[8 + i] * 977u + x[i];
    t[i] = (uint32_t)c;
    c >>= 32;
  }
  t[8] = (uint32_t)c;  // < 2^10
  c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)t[i + 1] + x[8 + i];
    t[i + 1] = (uint32_t)c;
    c >>= 32;
  }
  t[9] = (uint32_t)c;
  // fold 2: top = t[8..10) < 2^33; t[0..8) + top * (2^32 + 977)
  const uint64_t top = ((uint64_t)t[9] << 32) | t[8];
  const uint64_t m = top * 977u;  // < 2^43
  c = (uint64_t)t[0] + (uint32_t)m;
  t[0] = (uint32_t)c;
  c >>= 32;
  c += (uint64_t)t[1] + (uint32_t)(m >> 32) + (uint32_t)top;
  t[1] = (uint32_t)c;
  c >>= 32;
  c += (uint64_t)t[2] + (uint32_t)(top >> 32);
  t[2] = (uint32_t)c;
  c >>= 32;
#pragma unroll
  for (int i = 3; i < 8; i++) {
    c += t[i];
    t[i] = (uint32_t)c;
    c >>= 32;
  }
  // a carry out leaves t < 2^67: adding 2^32 + 977 for it cannot carry again
  const uint32_t k = (uint32_t)c;
  c = (uint64_t)t[0] + 977u * k;
  t[0] = (uint32_t)c;
  c >>= 32;
  c += (uint64_t)t[1] + k;
  t[1] = (uint32_t)c;
  c >>= 32;
#pragma unroll
  for (int i = 2; i < 8; i++) {
    c += t[i];
    t[i] = (uint32_t)c;
    c >>= 32;
  }
  fe_final(r, t, 0);
}
K1_HD void fe_mul(K1Fe& r, const K1Fe& a, const K1Fe& b) {
  uint32_t x[16];
  k1_mul512(x, a.v, b.v);
  fe_reduce512(r, x);
}
K1_HD void fe_sqr(K1Fe& r, const K1Fe& a) { fe_mul(r, a, a); }
K1_HD void fe_dbl(K1Fe& r, const K1Fe& a) { fe_add(r, a, a); }
// r = a^-1 (0 -> 0), variable time
K1_HD void fe_inv_var(K1Fe& r, const K1Fe& a) {
  Sg30 x;
  k1_to_s30(x, a.v);
  sg_inv30_var<K1FeS30>(x);
  k1_from_s30(r.v, x);
}
