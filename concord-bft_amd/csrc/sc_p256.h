// Arithmetic mod n, the order of P-256's group, for ECDSA verification (PUBLIC values only).
// Eight little-endian 32-bit limbs, canonical in [0, n).  Here 2^256 - n has 224 bits, so folding
// the high half down (sc_reduce512 of sc_secp256k1.h) gains 32 bits a round; the products are
// Montgomery's instead (word by word, R = 2^256), and a verification runs three of them and one
// inversion against ~3,000 field products in the point arithmetic.
#pragma once
#include "fe_p256.h"

struct P2Sc {
  uint32_t v[8];
};

#define P2_N_LIMBS                                                                                  \
  { 0xFC632551u, 0xF3B9CAC2u, 0xA7179E84u, 0xBCE6FAADu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0xFFFFFFFFu }
// R^2 mod n, R = 2^256
#define P2_N_RR_LIMBS                                                                               \
  { 0xBE79EEA2u, 0x83244C95u, 0x49BD6FA6u, 0x4699799Cu, 0x2B6BEC59u, 0x2845B239u, 0xF3D95620u, 0x66E12D94u }
// -n^-1 mod 2^32
#define P2_N_N0INV 0xEE00BC4Fu

struct P2ScS30 {  // n in signed-30 limbs, n^-1 mod 2^30
  static constexpr int32_t P[9] = {0x3c632551, 0x0ee72b0b, 0x3179e84f, 0x39beab69, 0x3fffffbc,
                                   0x3fffffff, 0x00000fff, 0x3fffc000, 0x0000ffff};
  static constexpr uint32_t PINV30 = 0x11ff43b1u;
};

K1_HD bool p2_sc_is_zero(const P2Sc& a) { return k1_is_zero256(a.v); }
// a < n
K1_HD bool p2_sc_in_range(const uint32_t* a) {
  const uint32_t N[8] = P2_N_LIMBS;
  uint32_t u[8];
  return k1_sub256(u, a, N) != 0;
}
// a < 2^256 -> a mod n (one subtraction: 2^256 < 2 n)
K1_HD void p2_sc_reduce256(P2Sc& r, const uint32_t* a) {
  const uint32_t N[8] = P2_N_LIMBS;
  uint32_t u[8];
  const uint32_t take = k1_sub256(u, a, N) ? 0u : 0xFFFFFFFFu;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (u[i] & take) | (a[i] & ~take);
}
// r = a b / 2^256 mod n for any a < 2^256 and b < n (coarsely integrated operand scanning).
// Bound: the accumulator t[0..9) is at most 2 n - 1 before every row (0 before the first): a row
// adds a[i] b + m n <= (2^32 - 1) (2 n - 1) and divides by 2^32 exactly, which maps [0, 2 n - 1] into
// itself.  So t[8] is 0 or 1 between rows, t + a[i] b < (2^32 + 1) n < 2^288 fits the nine words with no
// carry out of t[8], t + a[i] b + m n < 2^289 is why the second pass's carry out of t[8] becomes the new
// t[8] after the shift by one word, and the last row leaves t < 2 n: one conditional subtraction.
K1_HD void p2_sc_montmul(P2Sc& r, const uint32_t* a, const uint32_t* b) {
  const uint32_t N[8] = P2_N_LIMBS;
  uint32_t t[9];
#pragma unroll
  for (int i = 0; i < 9; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      c += (uint64_t)a[i] * b[j] + t[j];
      t[j] = (uint32_t)c;
      c >>= 32;
    }
    t[8] += (uint32_t)c;  // no carry out: t + a[i] b < 2^288
    const uint32_t m = t[0] * P2_N_N0INV;
    c = (uint64_t)m * N[0] + t[0];  // low word is 0
    c >>= 32;
#pragma unroll
    for (int j = 1; j < 8; j++) {
      c += (uint64_t)m * N[j] + t[j];
      t[j - 1] = (uint32_t)c;
      c >>= 32;
    }
    c += t[8];
    t[7] = (uint32_t)c;
    t[8] = (uint32_t)(c >> 32);
  }
  uint32_t u[8];
  const uint32_t borrow = k1_sub256(u, t, N);
  const uint32_t take = (t[8] | (borrow ^ 1u)) ? 0xFFFFFFFFu : 0u;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (u[i] & take) | (t[i] & ~take);
}
// a -> a 2^256 mod n, for any a < 2^256
K1_HD void p2_sc_to_mont(P2Sc& r, const P2Sc& a) {
  const uint32_t RR[8] = P2_N_RR_LIMBS;
  p2_sc_montmul(r, a.v, RR);
}
// r = a b mod n for any a, b < 2^256
K1_HD void p2_sc_mul(P2Sc& r, const P2Sc& a, const P2Sc& b) {
  P2Sc bm, br;
  p2_sc_reduce256(br, b.v);
  p2_sc_to_mont(bm, br);  // b 2^256 mod n, below n
  p2_sc_montmul(r, a.v, bm.v);
}
// r = a^-1 mod n (0 -> 0), variable time: safegcd30.h
K1_HD void p2_sc_inv_var(P2Sc& r, const P2Sc& a) {
  Sg30 x;
  k1_to_s30(x, a.v);
  sg_inv30_var<P2ScS30>(x);
  k1_from_s30(r.v, x);
}
