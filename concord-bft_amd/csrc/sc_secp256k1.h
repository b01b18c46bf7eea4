// Arithmetic mod n, the order of secp256k1's group, for ECDSA verification (PUBLIC values only).
// Eight little-endian 32-bit limbs, canonical in [0, n).  A verification runs two products and one
// inversion here against ~3,000 field products in the point arithmetic, so the reduction is the
// plain one: n = 2^256 - c with c < 2^129, fold the high half down with c until it is gone.
#pragma once
#include "fe_secp256k1.h"

struct K1Sc {
  uint32_t v[8];
};

#define K1_N_LIMBS                                                                                  \
  { 0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu }
// c = 2^256 - n
#define K1_NC_LIMBS \
  { 0x2FC9BEBFu, 0x402DA173u, 0x50B75FC4u, 0x45512319u, 0x00000001u }

struct K1ScS30 {  // n in signed-30 limbs, n^-1 mod 2^30
  static constexpr int32_t P[9] = {0x10364141, 0x3f497a33, 0x348a03bb, 0x2bb739ab, 0x3ffffeba,
                                   0x3fffffff, 0x3fffffff, 0x3fffffff, 0x0000ffff};
  static constexpr uint32_t PINV30 = 0x2a774ec1u;
};

K1_HD bool sc_is_zero(const K1Sc& a) { return k1_is_zero256(a.v); }
// a < n
K1_HD bool sc_in_range(const uint32_t* a) {
  const uint32_t N[8] = K1_N_LIMBS;
  uint32_t u[8];
  return k1_sub256(u, a, N) != 0;
}
// a < 2^256 -> a mod n (one subtraction: 2^256 < 2 n)
K1_HD void sc_reduce256(K1Sc& r, const uint32_t* a) {
  const uint32_t N[8] = K1_N_LIMBS;
  uint32_t u[8];
  const uint32_t take = k1_sub256(u, a, N) ? 0u : 0xFFFFFFFFu;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (u[i] & take) | (a[i] & ~take);
}
// x[0..16) -> x mod n.  Each round replaces hi 2^256 + lo by hi c + lo:
//   x < 2^512 -> < 2^386 -> < 2^260 -> < 2^256 + 2^133 (hi <= 1) -> hi = 0 (hi = 1 left lo < 2^133)
K1_HD void sc_reduce512(K1Sc& r, const uint32_t* x) {
  const uint32_t C[5] = K1_NC_LIMBS;
  uint32_t t[16];
#pragma unroll
  for (int i = 0; i < 16; i++) t[i] = x[i];
#pragma unroll 1
  for (int round = 0; round < 4; round++) {
    uint32_t u[16];
#pragma unroll
    for (int i = 0; i < 16; i++) u[i] = i < 8 ? t[i] : 0u;
#pragma unroll
    for (int i = 0; i < 8; i++) {  // u += hi[i] * c << 32 i ; the sum stays below 2^416
      uint64_t c = 0;
#pragma unroll
      for (int j = 0; j < 5; j++) {
        c += (uint64_t)t[8 + i] * C[j] + u[i + j];
        u[i + j] = (uint32_t)c;
        c >>= 32;
      }
#pragma unroll
      for (int k = i + 5; k < 14; k++) {
        c += u[k];
        u[k] = (uint32_t)c;
        c >>= 32;
      }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) t[i] = u[i];
  }
  sc_reduce256(r, t);
}
K1_HD void sc_mul(K1Sc& r, const K1Sc& a, const K1Sc& b) {
  uint32_t x[16];
  k1_mul512(x, a.v, b.v);
  sc_reduce512(r, x);
}
// r = a^-1 mod n (0 -> 0), variable time: safegcd30.h
K1_HD void sc_inv_var(K1Sc& r, const K1Sc& a) {
  Sg30 x;
  k1_to_s30(x, a.v);
  sg_inv30_var<K1ScS30>(x);
  k1_from_s30(r.v, x);
}
