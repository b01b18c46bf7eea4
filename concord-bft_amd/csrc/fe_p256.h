// GF(p), p = 2^256 - 2^224 + 2^192 + 2^96 - 1 (NIST P-256), for ECDSA verification: everything
// here works on PUBLIC values and may branch on them.  Eight little-endian 32-bit limbs, always
// canonical (in [0, p)), so equality and zero tests are exact word compares.  Products on the
// INT32 VALU (k1_mul512 of fe_secp256k1.h: one v_mad_u64_u32 per partial product); the reduction
// is the word-wise Solinas sum of FIPS 186-4 D.2.3, which has no multiply at all: signed 64-bit
// column sums of the product's words, then the carry out folded back with
// 2^256 = 2^224 - 2^192 - 2^96 + 1 (mod p).  Host and device from one source.
#pragma once
#include "fe_secp256k1.h"  // K1_HD, the 256-bit helpers (k1_add256 .. k1_from_s30), safegcd30.h

struct P2Fe {
  uint32_t v[8];
};

#define P2_P_LIMBS                                                                                  \
  { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000001u, 0xFFFFFFFFu }

struct P2FeS30 {  // p in signed-30 limbs, p^-1 mod 2^30
  static constexpr int32_t P[9] = {0x3fffffff, 0x3fffffff, 0x3fffffff, 0x0000003f, 0x00000000,
                                   0x00000000, 0x00001000, 0x3fffc000, 0x0000ffff};
  static constexpr uint32_t PINV30 = 0x3fffffffu;
};

K1_HD void p2_fe_zero(P2Fe& r) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = 0;
}
K1_HD void p2_fe_one(P2Fe& r) {
  p2_fe_zero(r);
  r.v[0] = 1;
}
K1_HD bool p2_fe_is_zero(const P2Fe& a) { return k1_is_zero256(a.v); }
K1_HD bool p2_fe_eq(const P2Fe& a, const P2Fe& b) { return k1_eq256(a.v, b.v); }

// t < 2^256 (+ carry 2^256) -> t mod p, given t + carry 2^256 < 2 p
K1_HD void p2_fe_final(P2Fe& r, const uint32_t* t, uint32_t carry) {
  const uint32_t P[8] = P2_P_LIMBS;
  uint32_t u[8];
  const uint32_t borrow = k1_sub256(u, t, P);
  const uint32_t take = (carry | (borrow ^ 1u)) ? 0xFFFFFFFFu : 0u;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (u[i] & take) | (t[i] & ~take);
}
// 32 big-endian bytes -> r; false (r unspecified) unless the value is below p
K1_HD bool p2_fe_from_be(P2Fe& r, const uint8_t* b) {
  const uint32_t P[8] = P2_P_LIMBS;
  uint32_t u[8];
  k1_from_be(r.v, b);
  return k1_sub256(u, r.v, P) != 0;
}
K1_HD void p2_fe_add(P2Fe& r, const P2Fe& a, const P2Fe& b) {
  uint32_t t[8];
  const uint32_t c = k1_add256(t, a.v, b.v);
  p2_fe_final(r, t, c);
}
K1_HD void p2_fe_sub(P2Fe& r, const P2Fe& a, const P2Fe& b) {
  const uint32_t P[8] = P2_P_LIMBS;
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
K1_HD void p2_fe_neg(P2Fe& r, const P2Fe& a) {
  P2Fe z;
  p2_fe_zero(z);
  p2_fe_sub(r, z, a);
}

// t[0..8) += k (2^224 - 2^192 - 2^96 + 1) for a small signed k; returns the signed carry out
K1_HD int64_t p2_fold(uint32_t* t, int64_t k) {
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (int64_t)t[i];
    if (i == 0 || i == 7) c += k;
    if (i == 3 || i == 6) c -= k;
    t[i] = (uint32_t)c;
    c >>= 32;  // arithmetic: the carry is signed
  }
  return c;
}

// x[0..16) -> x mod p.  With the product's words c0..c15, FIPS 186-4 D.2.3 gives
//   x = s1 + 2 s2 + 2 s3 + s4 + s5 - s6 - s7 - s8 - s9 (mod p)
// for nine 256-bit values made of those words; column i below is the sum of their i-th words.
// Bounds: a column holds at most 7 positive and 4 negative words (|column| < 2^35), the running
// carry stays below 2^4 in magnitude, so every int64 sum is far from overflow.  The value is
// t + k 2^256 with t in [0, 2^256) and -4 <= k <= 6 (four values subtracted, seven added).
// Fold 1 replaces k 2^256 by k (2^224 - 2^192 - 2^96 + 1), |that| < 6 * 2^224, leaving a carry k2
// in {-1, 0, 1}.  Fold 2: k2 = 1 means t < 6 * 2^224 and adding 2^224 - .. cannot carry; k2 = -1
// means t > 2^256 - 6 * 2^224 and subtracting it cannot borrow.  The result is in [0, 2^256)
// (below 2 p): one conditional subtraction of p finishes.
K1_HD void p2_fe_reduce512(P2Fe& r, const uint32_t* x) {
#define P2C(i) ((int64_t)x[i])
  uint32_t t[8];
  int64_t c;
  c = P2C(0) + P2C(8) + P2C(9) - P2C(11) - P2C(12) - P2C(13) - P2C(14);
  t[0] = (uint32_t)c;
  c >>= 32;
  c += P2C(1) + P2C(9) + P2C(10) - P2C(12) - P2C(13) - P2C(14) - P2C(15);
  t[1] = (uint32_t)c;
  c >>= 32;
  c += P2C(2) + P2C(10) + P2C(11) - P2C(13) - P2C(14) - P2C(15);
  t[2] = (uint32_t)c;
  c >>= 32;
  c += P2C(3) + 2 * P2C(11) + 2 * P2C(12) + P2C(13) - P2C(15) - P2C(8) - P2C(9);
  t[3] = (uint32_t)c;
  c >>= 32;
  c += P2C(4) + 2 * P2C(12) + 2 * P2C(13) + P2C(14) - P2C(9) - P2C(10);
  t[4] = (uint32_t)c;
  c >>= 32;
  c += P2C(5) + 2 * P2C(13) + 2 * P2C(14) + P2C(15) - P2C(10) - P2C(11);
  t[5] = (uint32_t)c;
  c >>= 32;
  c += P2C(6) + 3 * P2C(14) + 2 * P2C(15) + P2C(13) - P2C(8) - P2C(9);
  t[6] = (uint32_t)c;
  c >>= 32;
  c += P2C(7) + 3 * P2C(15) + P2C(8) - P2C(10) - P2C(11) - P2C(12) - P2C(13);
  t[7] = (uint32_t)c;
  c >>= 32;
#undef P2C
  c = p2_fold(t, c);
  (void)p2_fold(t, c);
  p2_fe_final(r, t, 0);
}
K1_HD void p2_fe_mul(P2Fe& r, const P2Fe& a, const P2Fe& b) {
  uint32_t x[16];
  k1_mul512(x, a.v, b.v);
  p2_fe_reduce512(r, x);
}
K1_HD void p2_fe_sqr(P2Fe& r, const P2Fe& a) { p2_fe_mul(r, a, a); }
K1_HD void p2_fe_dbl(P2Fe& r, const P2Fe& a) { p2_fe_add(r, a, a); }
// r = a^-1 (0 -> 0), variable time
K1_HD void p2_fe_inv_var(P2Fe& r, const P2Fe& a) {
  Sg30 x;
  k1_to_s30(x, a.v);
  sg_inv30_var<P2FeS30>(x);
  k1_from_s30(r.v, x);
}
