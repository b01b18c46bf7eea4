// Batched BLS key derivation on BN-P254 G2, one key per lane, and Shamir dealing in Fr.
//
//   vk = (sk mod r) * g2, compressed                       (BlsThresholdSigner's publicKey_)
//   sk_i = f(i) = sum_j c_j i^j mod r, i = 1..n            (BlsThresholdKeygen.cpp:28-50)
//
// The lane-level routines below are one-lane BN_HD code (bn254_field.h), so the same source runs on
// gfx950 (bls_keygen_batch.hip) and on the host (tests/cpp/bls_keygen_shim.cpp).  Everything that
// touches a scalar, a coefficient or a value derived from them runs a fixed instruction sequence: no
// address, branch, loop bound or choice of load depends on it.  The comb table of g2, the share ids and
// the finished keys are public; whether a scalar is 0 mod r is published by the call itself (ok = 0).
#pragma once
#include "bls_sign_batch.h"

// ------------------------------------------------------------------------------ Fp2, secret operands
// the forms of bn254_tower.h on f_add_ct / f_sub_ct: the same limbs, no branch on the operands
BN_HD void fp2_add_ct(fp2& r, const fp2& x, const fp2& y) {
  f_add_ct(r.a, x.a, y.a);
  f_add_ct(r.b, x.b, y.b);
}
BN_HD void fp2_sub_ct(fp2& r, const fp2& x, const fp2& y) {
  f_sub_ct(r.a, x.a, y.a);
  f_sub_ct(r.b, x.b, y.b);
}
BN_HD void fp2_neg_ct(fp2& r, const fp2& x) {
  fp z;
  f_zero(z);
  f_sub_ct(r.a, z, x.a);
  f_sub_ct(r.b, z, x.b);
}
BN_HD void fp2_mul_ct(fp2& r, const fp2& x, const fp2& y) {  // Karatsuba, 3 M (fp2_mul)
  fp t0, t1, s0, s1;
  f_mul(t0, x.a, y.a);
  f_mul(t1, x.b, y.b);
  f_add_ct(s0, x.a, x.b);
  f_add_ct(s1, y.a, y.b);
  f_mul(s0, s0, s1);
  f_sub_ct(r.a, t0, t1);
  f_sub_ct(s0, s0, t0);
  f_sub_ct(r.b, s0, t1);
}
BN_HD void fp2_sqr_ct(fp2& r, const fp2& x) {  // complex squaring, 2 M (fp2_sqr)
  fp s, d, m;
  f_add_ct(s, x.a, x.b);
  f_sub_ct(d, x.a, x.b);
  f_mul(m, x.a, x.b);
  f_mul(r.a, s, d);
  f_add_ct(r.b, m, m);
}
BN_HD void fp2_sel_ct(fp2& r, uint32_t m, const fp2& a, const fp2& b) {  // m ? a : b
  f_sel_ct(r.a, m, a.a, b.a);
  f_sel_ct(r.b, m, a.b, b.b);
}

// ------------------------------------------------------------------------------ scalars mod r
// r as 8 little-endian words
struct BlsKgR {
  static constexpr uint32_t W[8] = {0x0000000du, 0xa1000000u, 0x00000010u, 0xff9f8000u,
                                    0x00000007u, 0xba344d80u, 0x40000001u, 0x25236482u};
};
// k -= (r << sh) where k >= (r << sh), by a mask (r << 2 < 2^256)
BN_HD void bls_kg_csub_r(uint32_t* k, int sh) {
  uint32_t t[8];
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t lo = BlsKgR::W[i] << sh;
    const uint32_t hi = (i && sh) ? BlsKgR::W[i - 1] >> (32 - sh) : 0u;
    const int64_t d = (int64_t)k[i] - (int64_t)(lo | hi) + br;
    t[i] = (uint32_t)d;
    br = d >> 32;
  }
  const uint32_t keep = bls_opaque(~(uint32_t)br);  // no borrow: the difference stands
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = (t[i] & keep) | (k[i] & ~keep);
}
// any 256-bit value (< 2^256 < 7 r) -> [0, r): 4r, 2r and r come off where they fit
BN_HD void bls_kg_reduce(uint32_t* k) {
  bls_kg_csub_r(k, 2);
  bls_kg_csub_r(k, 1);
  bls_kg_csub_r(k, 0);
}
BN_HD uint32_t bls_kg_zero_mask(const uint32_t* k) {  // all ones iff k == 0
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) d |= k[i];
  return bls_opaque(~(uint32_t)((int32_t)(d | (0u - d)) >> 31));
}

// ------------------------------------------------------------------------------ the comb of g2
// PUB_T[j][e] = (2e + 1) 16^j g2, affine, canonical Montgomery limbs x.a | x.b | y.a | y.b: the table
// bls_keys.hip builds once per context (bls_pub_table_kernel) and the lone cbft_bls_public_key reads.
#define BLS_KG_POS 64
#define BLS_KG_ENT 8
#define BLS_KG_WORDS 36
#define BLS_KG_TBL_WORDS (BLS_KG_POS * BLS_KG_ENT * BLS_KG_WORDS)

// the same table by plain (branching) public arithmetic: the host build's table, and the check of the
// device table
BN_HDN void bls_kg_table_position(uint32_t* tbl, int j) {
  g2j P;
  fp2_load(P.X, Bn254Consts::G2X);
  fp2_load(P.Y, Bn254Consts::G2Y);
  fp2_one(P.Z);
  for (int d = 0; d < 4 * j; d++) {
    g2j t;
    g2_dbl_j(t, P);
    P = t;
  }
  g2j P2, E = P;
  g2_dbl_j(P2, P);
  for (int e = 0; e < BLS_KG_ENT; e++) {
    if (e) {
      g2j t;
      g2_add_j(t, E, P2);
      E = t;
    }
    g2a a;
    g2_to_affine(a, E);
    f_canon(a.x.a);
    f_canon(a.x.b);
    f_canon(a.y.a);
    f_canon(a.y.b);
    uint32_t* o = tbl + ((size_t)j * BLS_KG_ENT + e) * BLS_KG_WORDS;
    for (int i = 0; i < BN_LIMBS; i++) {
      o[i] = a.x.a.v[i];
      o[9 + i] = a.x.b.v[i];
      o[18 + i] = a.y.a.v[i];
      o[27 + i] = a.y.b.v[i];
    }
  }
}

// (x, y) = +-PUB_T[j][(|d| - 1) / 2] for the digit d = 2 nib - 15: all 8 entries of the position are
// read (the address depends on j alone, the same in every lane), one is kept by masks, the sign by a
// mask
BN_HD void bls_kg_pick(fp2& x, fp2& y, const uint32_t* tbl, int j, uint32_t nib) {
  const uint32_t dn = 0u - ((nib >> 3) ^ 1u);  // d < 0 (nib < 8)
  const uint32_t m = (nib ^ dn) & 7u;          // nib - 8, or 7 - nib
  const uint32_t* base = tbl + (size_t)j * BLS_KG_ENT * BLS_KG_WORDS;
  uint32_t w[BLS_KG_WORDS];
#pragma unroll
  for (int i = 0; i < BLS_KG_WORDS; i++) w[i] = 0;
#pragma unroll
  for (int e = 0; e < BLS_KG_ENT; e++) {
    const uint32_t hit = bls_opaque((uint32_t)((int32_t)((m ^ (uint32_t)e) - 1u) >> 31));
#pragma unroll
    for (int i = 0; i < BLS_KG_WORDS; i++) w[i] |= base[e * BLS_KG_WORDS + i] & hit;
  }
#pragma unroll
  for (int i = 0; i < BN_LIMBS; i++) {
    x.a.v[i] = w[i];
    x.b.v[i] = w[9 + i];
    y.a.v[i] = w[18 + i];
    y.b.v[i] = w[27 + i];
  }
  fp2 ny;
  fp2_neg_ct(ny, y);
  fp2_sel_ct(y, bls_opaque(dn), ny, y);
}

// INCOMPLETE mixed addition (madd-2007-bl without its case analysis): acc += (x, y), right for a finite
// acc != +-(x, y).  The comb below never leaves that domain.
BN_HDN void g2_madd_ct(g2j& acc, const fp2& x, const fp2& y) {
  fp2 Z1Z1, U2, S2, H, HH, I, J, rr, V, t, X3, Y3, Z3;
  fp2_sqr_ct(Z1Z1, acc.Z);
  fp2_mul_ct(U2, x, Z1Z1);
  fp2_mul_ct(S2, y, acc.Z);
  fp2_mul_ct(S2, S2, Z1Z1);
  fp2_sub_ct(H, U2, acc.X);
  fp2_sqr_ct(HH, H);
  fp2_add_ct(I, HH, HH);
  fp2_add_ct(I, I, I);
  fp2_mul_ct(J, H, I);
  fp2_sub_ct(rr, S2, acc.Y);
  fp2_add_ct(rr, rr, rr);
  fp2_mul_ct(V, acc.X, I);
  fp2_sqr_ct(X3, rr);
  fp2_sub_ct(X3, X3, J);
  fp2_sub_ct(X3, X3, V);
  fp2_sub_ct(X3, X3, V);
  fp2_sub_ct(t, V, X3);
  fp2_mul_ct(Y3, rr, t);
  fp2_mul_ct(t, acc.Y, J);
  fp2_add_ct(t, t, t);
  fp2_sub_ct(Y3, Y3, t);
  fp2_add_ct(Z3, acc.Z, H);
  fp2_sqr_ct(Z3, Z3);
  fp2_sub_ct(Z3, Z3, Z1Z1);
  fp2_sub_ct(Z3, Z3, HH);
  acc.X = X3;
  acc.Y = Y3;
  acc.Z = Z3;
}

// out65 = compress((k mod r) g2), *ok = 1; k = 0 mod r: 65 zero bytes, *ok = 0.  k: 8 little-endian
// words, any 256-bit value (clobbered).  tbl: the comb above.
//
// Scheme (the lone kernel's, bls_keys.hip bls_pubkey_row_kernel, one key per lane).  k is reduced;
// 0 is replaced by 1 (mask) and its output blanked at the end.  An even k is replaced by the odd
// k' = r - k and the result negated, both by masks, so k' is odd in [1, r - 1].  With
// u = (k' + 2^256 - 1) / 2 and nib_j its radix-16 digits, d_j = 2 nib_j - 15 are odd, |d_j| <= 15, and
// sum_j d_j 16^j = 2u - (16^64 - 1) = k'.  The key is PUB_T[0][.] plus 63 mixed additions, position 0
// upwards.
//
// Why no addition is exceptional.  Before position j the accumulator is S g2 with S = sum_{i<j} d_i 16^i
// odd, |S| < 16^j, and the addend is A g2, A = d_j 16^j, |A| >= 16^j.  For j <= 62, |S +- A| lies in
// [1, 16^63) and 16^63 = 2^252 < r, so S != +-A mod r and neither point is infinity.  For j = 63,
// u < 2^255 + 2^253 makes nib_63 in {8, 9}, A in {1, 3} 2^252: S + A = k' is in [1, r - 1], not 0 mod r;
// S - A is in (-2^254, 0) and r > 2^253, so S = A mod r only if S = A - r, and then k' = 2A - r, which for
// A = 2^252 is negative and for A = 3 2^252 is 3 2^253 - r > r (r < 1.17 2^253): neither is a k'.
//
// Affine conversion: a constant-time Fermat inversion of Z's norm in this lane (fp_inv: a fixed
// square-and-multiply over the public exponent p - 2), so no lane's Z meets another's.  The affine
// point is the public key.
BN_HD void bls_keygen_lane(uint8_t* out65, uint8_t* ok, uint32_t* k, const uint32_t* tbl) {
  bls_kg_reduce(k);
  const uint32_t zero = bls_kg_zero_mask(k);
  k[0] |= zero & 1u;
  const uint32_t emask = bls_opaque(0u - ((k[0] & 1u) ^ 1u));
  {
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int64_t d = (int64_t)BlsKgR::W[i] - k[i] + br;
      k[i] = ((uint32_t)d & emask) | (k[i] & ~emask);
      br = d >> 32;
    }
  }
  uint32_t u[8];
  {  // u = (k' + 2^256 - 1) / 2
    uint64_t cy = 0;
    uint32_t t[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      cy += (uint64_t)k[i] + 0xffffffffu;
      t[i] = (uint32_t)cy;
      cy >>= 32;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) u[i] = (t[i] >> 1) | (i < 7 ? (t[i + 1] << 31) : ((uint32_t)cy << 31));
  }
  g2j acc;
  bls_kg_pick(acc.X, acc.Y, tbl, 0, u[0] & 15u);
  fp2_one(acc.Z);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
  for (int j = 1; j < BLS_KG_POS; j++) {
    // the digit without a variable word index: u moves down a nibble per position
#pragma unroll
    for (int i = 0; i < 7; i++) u[i] = (u[i] >> 4) | (u[i + 1] << 28);
    u[7] >>= 4;
    fp2 x, y;
    bls_kg_pick(x, y, tbl, j, u[0] & 15u);
    g2_madd_ct(acc, x, y);
  }
  {  // k even: k g2 = -(r - k) g2
    fp2 ny;
    fp2_neg_ct(ny, acc.Y);
    fp2_sel_ct(acc.Y, emask, ny, acc.Y);
  }
  fp n, t;
  fp2 zi, zi2;
  f_sqr(n, acc.Z.a);
  f_sqr(t, acc.Z.b);
  f_add_ct(n, n, t);
  fp_inv(n, n);
  f_mul(zi.a, acc.Z.a, n);
  f_mul(t, acc.Z.b, n);
  {
    fp z;
    f_zero(z);
    f_sub_ct(zi.b, z, t);
  }
  g2a a;
  fp2_sqr_ct(zi2, zi);
  fp2_mul_ct(a.x, acc.X, zi2);
  fp2_mul_ct(zi2, zi2, zi);
  fp2_mul_ct(a.y, acc.Y, zi2);
  a.inf = false;
  uint8_t b[65];
  g2_compress(b, a);  // public from here on (but for the zero scalar's stand-in, blanked by the mask)
  const uint8_t keep = (uint8_t)~zero;
  for (int i = 0; i < 65; i++) out65[i] = b[i] & keep;
  *ok = (uint8_t)(1u & ~zero);
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = u[i] = 0;
}

// ------------------------------------------------------------------------------ dealing in Fr
// fr's f_mul / f_sqr have no branch (f_redc); f_add / f_sub do, so sums go through f_add_ct.
// canonical [0, r) from a reduced element (< 2r), by a mask (f_canon selects on a condition)
BN_HD void fr_canon_ct(fr& a) {
  uint32_t t[BN_LIMBS];
  int32_t br = 0;
#pragma unroll
  for (int i = 0; i < BN_LIMBS; i++) {
    const int32_t d = (int32_t)a.v[i] - (int32_t)FrParams::Q[i] + br;
    t[i] = (uint32_t)d & BN_MASK;
    br = d >> 29;
  }
  const uint32_t keep = bls_opaque(~(uint32_t)br);
#pragma unroll
  for (int i = 0; i < BN_LIMBS; i++) a.v[i] = (t[i] & keep) | (a.v[i] & ~keep);
}
// Montgomery form of a 32-byte big-endian coefficient, any 256-bit value (reduced first)
BN_HD void bls_kg_coeff(fr& c, const uint8_t* be32) {
  uint32_t w[8];
  be32_to_words(w, be32);
  bls_kg_reduce(w);
  f_from_words(c, w);
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = 0;
}
// Montgomery -> canonical integer words, masks only (f_to_words with fr_canon_ct)
BN_HD void bls_kg_fr_words(uint32_t* w, const fr& a) {
  fr one, t;
  f_zero(one);
  one.v[0] = 1;
  f_mul(t, a, one);
  fr_canon_ct(t);
  w[0] = t.v[0] | (t.v[1] << 29);
  w[1] = (t.v[1] >> 3) | (t.v[2] << 26);
  w[2] = (t.v[2] >> 6) | (t.v[3] << 23);
  w[3] = (t.v[3] >> 9) | (t.v[4] << 20);
  w[4] = (t.v[4] >> 12) | (t.v[5] << 17);
  w[5] = (t.v[5] >> 15) | (t.v[6] << 14);
  w[6] = (t.v[6] >> 18) | (t.v[7] << 11);
  w[7] = (t.v[7] >> 21) | (t.v[8] << 8);
}
// out32 = f(id) mod r, canonical big-endian, for the polynomial's k coefficients in Montgomery form
// (coeff[j * stride + limb]): Horner from the top coefficient, k - 1 multiplications by id.  The id and
// k are public; the coefficients and the accumulator are not.
BN_HD void bls_kg_eval_lane(uint8_t* out32, const uint32_t* coeff, size_t stride, uint32_t k, uint32_t id) {
  fr x, acc, c;
  {
    const uint32_t w[8] = {id, 0, 0, 0, 0, 0, 0, 0};
    f_from_words(x, w);
  }
#pragma unroll
  for (int i = 0; i < BN_LIMBS; i++) acc.v[i] = coeff[(size_t)(k - 1) * stride + i];
  for (uint32_t j = k - 1; j-- > 0;) {
#pragma unroll
    for (int i = 0; i < BN_LIMBS; i++) c.v[i] = coeff[(size_t)j * stride + i];
    f_mul(acc, acc, x);
    f_add_ct(acc, acc, c);
  }
  uint32_t w[8];
  bls_kg_fr_words(w, acc);
  words_to_be32(out32, w);
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = 0;
}

// ------------------------------------------------------------------------------ launches (bls_keygen_batch.hip)
#if defined(__HIPCC__)
// keys per launch
#define BLS_KEYGEN_LAUNCH_MAX (1u << 20)
// d_out65 = n x 65, d_ok = n (nullable), from n x 32 big-endian scalar bytes (d_sk32) or, where that is
// null, n x 8 little-endian scalar words (d_skw: a signer table's staging); d_tbl: the context's comb of g2
hipError_t cbft_bls_keygen_launch(const uint32_t* d_tbl, const uint8_t* d_sk32, const uint32_t* d_skw, uint32_t n,
                                  uint8_t* d_out65, uint8_t* d_ok, hipStream_t s);
// Shamir dealing: d_coeff32 = k x 32 bytes; d_mont = k x BN_LIMBS words of scratch (secret); d_sk32 =
// (n + 1) x 32 bytes: [0] = c_0 mod r, [i] = f(i), canonical big-endian
hipError_t cbft_bls_keygen_launch_deal(const uint8_t* d_coeff32, uint32_t k, uint32_t n, uint32_t* d_mont,
                                       uint8_t* d_sk32, hipStream_t s);
#endif
