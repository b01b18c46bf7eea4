// Batched BLS share signing on BN-P254 G1, one message per lane.
//
//   share = be32(id) || compress(sk * g1_map(msg))          (BlsThresholdSigner.cpp:32-47)
//
// The lane-level routines below are one-lane BN_HD code (bn254_field.h), so the same source runs
// on gfx950 (bls_sign_batch.hip) and on the host (tests/cpp/bls_sign_shim.cpp).  Everything that
// touches the scalar or a value derived from it runs a fixed instruction sequence: no address,
// branch, loop bound or choice of load depends on it.  The message, its hash point H and the
// table of H's odd multiples are public; so is the finished share.
#pragma once
#include "bls_ops.h"

// ------------------------------------------------------------------------------ field, secret operands
// f_add / f_sub (bn254_field.h) run their correction pass only when some lane needs it: a wave-level
// branch on the operands.  These forms always run it (masked), and give the same limbs.
template <class F>
BN_HD void f_fix_2q_ct(Fe<F>& r, int32_t c /* 0 or -1: the pass went negative */) {
  uint32_t q2[BN_LIMBS];
  f_2q<F>(q2);
  const uint32_t msk = (uint32_t)(c >> 31) & BN_MASK;
  uint32_t cy = 0;
#pragma unroll
  for (int i = 0; i < BN_LIMBS; i++) {
    const uint32_t x = r.v[i] + (q2[i] & msk) + cy;
    r.v[i] = x & BN_MASK;
    cy = x >> 29;
  }
}
template <class F>
BN_HD void f_add_ct(Fe<F>& r, const Fe<F>& a, const Fe<F>& b) {
  uint32_t q2[BN_LIMBS];
  f_2q<F>(q2);
  const uint32_t t = a.v[BN_LIMBS - 1] + b.v[BN_LIMBS - 1];
  const uint32_t msk = (0u - (uint32_t)(t + 2 > q2[BN_LIMBS - 1])) & BN_MASK;
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < BN_LIMBS; i++) {
    const int32_t x = (int32_t)(a.v[i] + b.v[i]) - (int32_t)(q2[i] & msk) + c;
    r.v[i] = (uint32_t)x & BN_MASK;
    c = x >> 29;
  }
  f_fix_2q_ct(r, c);
}
template <class F>
BN_HD void f_sub_ct(Fe<F>& r, const Fe<F>& a, const Fe<F>& b) {
  uint32_t q2[BN_LIMBS];
  f_2q<F>(q2);
  const uint32_t msk = (0u - (uint32_t)(a.v[BN_LIMBS - 1] < b.v[BN_LIMBS - 1])) & BN_MASK;
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < BN_LIMBS; i++) {
    const int32_t x = (int32_t)a.v[i] - (int32_t)b.v[i] + (int32_t)(q2[i] & msk) + c;
    r.v[i] = (uint32_t)x & BN_MASK;
    c = x >> 29;
  }
  f_fix_2q_ct(r, c);
}

// a mask (all ones / zero) the compiler cannot turn back into a condition (ed25519_sign.h sign_opaque)
BN_HD uint32_t bls_opaque(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(m));
#endif
  return m;
}
// all ones iff a == 0 mod q (a < 2q, normalised): a is 0 or q limb for limb
template <class F>
BN_HD uint32_t f_zero_mask_ct(const Fe<F>& a) {
  uint32_t d0 = 0, dq = 0;
#pragma unroll
  for (int i = 0; i < BN_LIMBS; i++) {
    d0 |= a.v[i];
    dq |= a.v[i] ^ F::Q[i];
  }
  const uint32_t z0 = ~(uint32_t)((int32_t)(d0 | (0u - d0)) >> 31);  // d0 == 0 -> ~0, else 0
  const uint32_t zq = ~(uint32_t)((int32_t)(dq | (0u - dq)) >> 31);
  return bls_opaque(z0 | zq);
}
template <class F>
BN_HD void f_sel_ct(Fe<F>& r, uint32_t m, const Fe<F>& a, const Fe<F>& b) {  // m ? a : b
#pragma unroll
  for (int i = 0; i < BN_LIMBS; i++) r.v[i] = (a.v[i] & m) | (b.v[i] & ~m);
}

// ------------------------------------------------------------------------------ G1, secret operands
BN_HD void g1_sel_ct(g1j& r, uint32_t m, const g1j& a, const g1j& b) {
  f_sel_ct(r.X, m, a.X, b.X);
  f_sel_ct(r.Y, m, a.Y, b.Y);
  f_sel_ct(r.Z, m, a.Z, b.Z);
}

// g1_dbl (dbl-2009-l, a = 0) on the branch-free field forms; p = infinity (Z = 0) gives Z = 0
BN_HDN void g1_dbl_ct(g1j& r, const g1j& p) {
  fp A, B, C, D, E, F, t, Z3;
  f_sqr(A, p.X);
  f_sqr(B, p.Y);
  f_sqr(C, B);
  f_add_ct(t, p.X, B);
  f_sqr(t, t);
  f_sub_ct(t, t, A);
  f_sub_ct(t, t, C);
  f_add_ct(D, t, t);
  f_add_ct(E, A, A);
  f_add_ct(E, E, A);
  f_sqr(F, E);
  f_mul(Z3, p.Y, p.Z);
  f_add_ct(r.Z, Z3, Z3);
  f_sub_ct(r.X, F, D);
  f_sub_ct(r.X, r.X, D);
  f_sub_ct(t, D, r.X);
  f_mul(t, E, t);
  f_add_ct(C, C, C);
  f_add_ct(C, C, C);
  f_add_ct(C, C, C);
  f_sub_ct(r.Y, t, C);
}

// INCOMPLETE Jacobian addition (add-2007-bl without its case analysis): right for p != +-q, both
// finite.  For p = q it returns (0, 0, 0); hz / rz report H = 0 (same x) and r = 0 (same y) as masks so
// that a caller which can meet those cases decides by selects.
BN_HDN void g1_add_ct(g1j& r, const g1j& p, const g1j& q, uint32_t& hz, uint32_t& rz) {
  fp Z1Z1, Z2Z2, U1, U2, S1, S2, H, I, J, rr, V, t, X3, Y3, Z3;
  f_sqr(Z1Z1, p.Z);
  f_sqr(Z2Z2, q.Z);
  f_mul(U1, p.X, Z2Z2);
  f_mul(U2, q.X, Z1Z1);
  f_mul(S1, p.Y, q.Z);
  f_mul(S1, S1, Z2Z2);
  f_mul(S2, q.Y, p.Z);
  f_mul(S2, S2, Z1Z1);
  f_sub_ct(H, U2, U1);
  f_sub_ct(rr, S2, S1);
  hz = f_zero_mask_ct(H);
  rz = f_zero_mask_ct(rr);
  f_add_ct(I, H, H);
  f_sqr(I, I);
  f_mul(J, H, I);
  f_add_ct(rr, rr, rr);
  f_mul(V, U1, I);
  f_sqr(X3, rr);
  f_sub_ct(X3, X3, J);
  f_sub_ct(X3, X3, V);
  f_sub_ct(X3, X3, V);
  f_sub_ct(t, V, X3);
  f_mul(Y3, rr, t);
  f_mul(t, S1, J);
  f_add_ct(t, t, t);
  f_sub_ct(Y3, Y3, t);
  f_add_ct(Z3, p.Z, q.Z);
  f_sqr(Z3, Z3);
  f_sub_ct(Z3, Z3, Z1Z1);
  f_sub_ct(Z3, Z3, Z2Z2);
  f_mul(r.Z, Z3, H);
  r.X = X3;
  r.Y = Y3;
}

// ------------------------------------------------------------------------------ signer record
// GLV: sk = k1 + k2 lam (mod r), the split of bls_glv.h / bls_msm_row.hip's glv_split_ct restated as
// BN_HD code (that header is device-only) with the same constants, signs by masks.
struct BlsGlvConsts {
  static constexpr uint32_t G1[3] = {0x8a6b4904u, 0x7937ca68u, 0x00000003u};
  static constexpr uint32_t G2[5] = {0x36bf3357u, 0xc0eb31ffu, 0x04a017b9u, 0xa01fab7eu, 0x00000002u};
  static constexpr uint32_t A1[2] = {0x00000001u, 0x81000000u};
  static constexpr uint32_t A2[4] = {0x00000004u, 0x85000000u, 0x00000002u, 0x61818000u};
  static constexpr uint32_t B1[4] = {0x00000003u, 0x04000000u, 0x00000002u, 0x61818000u};  // |b1|, b1 < 0
  static constexpr uint32_t B2[2] = {0x00000001u, 0x81000000u};
  static constexpr uint32_t BETA[8] = {0x00000007u, 0xcd800000u, 0x00000006u, 0x49090000u,
                                       0x00000002u, 0x49b36240u, 0x00000000u, 0x00000000u};
};

template <int NA, int NB, int NO>
BN_HD void bls_mp_mul(uint32_t* out, const uint32_t* a, const uint32_t* b, int shift) {
  uint32_t t[NA + NB];
#pragma unroll
  for (int i = 0; i < NA + NB; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < NA; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      c += (uint64_t)a[i] * b[j] + t[i + j];
      t[i + j] = (uint32_t)c;
      c >>= 32;
    }
    t[i + NB] = (uint32_t)c;
  }
#pragma unroll
  for (int i = 0; i < NO; i++) out[i] = (shift + i < NA + NB) ? t[shift + i] : 0u;
}
BN_HD void bls_mp_sub8(uint32_t* a, const uint32_t* b) {
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int64_t d = (int64_t)a[i] - b[i] + br;
    a[i] = (uint32_t)d;
    br = d >> 32;
  }
}
BN_HD void bls_mp_neg_ct(uint32_t* a, uint32_t m /* 0 or ~0 */) {
  uint64_t c = m & 1u;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint32_t)(a[i] ^ m);
    a[i] = (uint32_t)c;
    c >>= 32;
  }
}
// k (8 LE words, < r) -> |k1|, |k2| (5 words each, < 2^128) and their signs as masks
BN_HD void bls_glv_split_ct(const uint32_t* k, uint32_t* k1, uint32_t* k2, uint32_t& n1, uint32_t& n2) {
  uint32_t c1[3], c2[5], g1[3], g2[5], a1[2], a2[4], b1[4], b2[2];
#pragma unroll
  for (int i = 0; i < 3; i++) g1[i] = BlsGlvConsts::G1[i];
#pragma unroll
  for (int i = 0; i < 5; i++) g2[i] = BlsGlvConsts::G2[i];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    a1[i] = BlsGlvConsts::A1[i];
    b2[i] = BlsGlvConsts::B2[i];
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    a2[i] = BlsGlvConsts::A2[i];
    b1[i] = BlsGlvConsts::B1[i];
  }
  bls_mp_mul<8, 3, 3>(c1, k, g1, 8);
  bls_mp_mul<8, 5, 5>(c2, k, g2, 8);
  uint32_t t[8], p[8];
#pragma unroll
  for (int i = 0; i < 8; i++) t[i] = k[i];
  bls_mp_mul<3, 2, 8>(p, c1, a1, 0);
  bls_mp_sub8(t, p);
  bls_mp_mul<5, 4, 8>(p, c2, a2, 0);
  bls_mp_sub8(t, p);  // k1 = k - c1 a1 - c2 a2
  n1 = 0u - (t[7] >> 31);
  bls_mp_neg_ct(t, n1);
#pragma unroll
  for (int i = 0; i < 5; i++) k1[i] = t[i];
  bls_mp_mul<3, 4, 8>(t, c1, b1, 0);  // -c1 b1 = c1 |b1|
  bls_mp_mul<5, 2, 8>(p, c2, b2, 0);
  bls_mp_sub8(t, p);  // k2 = c1 |b1| - c2 b2
  n2 = 0u - (t[7] >> 31);
  bls_mp_neg_ct(t, n2);
#pragma unroll
  for (int i = 0; i < 5; i++) k2[i] = t[i];
}

// One signer's record, everything the per-signature kernel would otherwise redo per message:
//   words 0..4, 5..9  the two halves' recoded digit words: each half |k_h| is made odd (+1 when even,
//                     undone at the end) and u = (k + 2^132 - 1) / 2 is stored shifted left by 28 bits,
//                     so the odd signed digits pop off the top of word 4, most significant first:
//                     with W-bit groups g_w of u (W divides 132), d_w = 2 g_w - (2^W - 1) and
//                     sum d_w 2^(W w) = 2 u - (2^132 - 1) = k.  The same words serve W = 4 (33 radix-16
//                     digits, 8 table entries) and W = 3 (44 radix-8 digits, 4 entries);
//   word 10           bit 0 / 1: k1 / k2 negative, bit 2 / 3: the odd fix was applied to k1 / k2;
//   word 11           the share id.
#define BLS_SIGNER_WORDS 12
#define BLS_SIGN_BITS 132
#define BLS_SIGN_W 3  // the window the product runs; 4 is the measured alternative
#define BLS_SIGN_TBL_WORDS(W) ((1 << ((W) - 1)) * 3 * BN_LIMBS)  // W = 3: 108 words, W = 4: 216 words
BN_HD void bls_signer_record(uint32_t* rec, const uint32_t* k, uint32_t id) {
  uint32_t kk[2][5], n[2];
  bls_glv_split_ct(k, kk[0], kk[1], n[0], n[1]);
  uint32_t flags = (n[0] & 1u) | (n[1] & 2u);
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t even = (kk[h][0] & 1u) ^ 1u;
    flags |= even << (2 + h);
    uint64_t cy = even;
#pragma unroll
    for (int i = 0; i < 5; i++) {
      cy += kk[h][i];
      kk[h][i] = (uint32_t)cy;
      cy >>= 32;
    }
    uint32_t u[5];
    cy = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
      cy += (uint64_t)kk[h][i] + (i < 4 ? 0xffffffffu : 0xfu);
      u[i] = (uint32_t)cy;
      cy >>= 32;
    }
    // (u >> 1) << 28 = u << 27: bits 0..131 of u >> 1 land in bits 28..159
#pragma unroll
    for (int i = 4; i >= 0; i--) rec[5 * h + i] = (u[i] << 27) | (i ? (u[i - 1] >> 5) : 0u);
  }
  rec[10] = flags;
  rec[11] = id;
}

// ------------------------------------------------------------------------------ hash to G1 (public)
// g1_map (bls_ops.h) in two parts, so that a kernel can schedule the tries: x0 = SHA-256(msg) mod p,
// then one try per call
BN_HD void bls_map_x0(fp& x, const uint8_t* msg, uint32_t len) {
  uint8_t d[32];
  sha256(d, msg, len);
  uint32_t w[8];
  be32_to_words(w, d);
  f_from_words(x, w);
}
// y = sqrt(x^3 + 2) if there is one; else x <- x + 1 and false
BN_HD bool bls_map_try(fp& y, fp& x) {
  fp rhs, two, one;
  const uint32_t t[8] = {2, 0, 0, 0, 0, 0, 0, 0};
  f_from_words(two, t);
  f_sqr(rhs, x);
  f_mul(rhs, rhs, x);
  f_add(rhs, rhs, two);
  if (fp_sqrt(y, rhs)) return true;
  f_one(one);
  f_add(x, x, one);
  return false;
}

// ------------------------------------------------------------------------------ one signature
// Table storage policies give put(e, w, value) / get(e, w) for entry e < 8, word w < 27.
struct BlsTblLocal {  // plain array (host build)
  uint32_t t[BLS_SIGN_TBL_WORDS(4)];
  BN_HD void put(int e, int w, uint32_t v) { t[e * 27 + w] = v; }
  BN_HD uint32_t get(int e, int w) const { return t[e * 27 + w]; }
};
struct BlsTblStrided {  // [entry][word][lane stride]: coalesced across the lanes of a wave
  uint32_t* base;
  size_t stride;
  BN_HD void put(int e, int w, uint32_t v) { base[(size_t)(e * 27 + w) * stride] = v; }
  BN_HD uint32_t get(int e, int w) const { return base[(size_t)(e * 27 + w) * stride]; }
};

template <class Tbl>
BN_HD void bls_tbl_put(Tbl& tbl, int e, const g1j& p) {
#pragma unroll
  for (int i = 0; i < BN_LIMBS; i++) {
    tbl.put(e, i, p.X.v[i]);
    tbl.put(e, 9 + i, p.Y.v[i]);
    tbl.put(e, 18 + i, p.Z.v[i]);
  }
}

// e = +-T[(|d| - 1) / 2] for the digit d = 2 g - (2^W - 1), g the W bits on top of u (popped), the sign
// flipped where neg: EVERY entry is read, one is kept by masks; the sign by a mask.
template <int W, class Tbl>
BN_HD void bls_sign_pick(g1j& e, uint32_t* u, uint32_t neg, const Tbl& tbl) {
  constexpr uint32_t E = 1u << (W - 1);
  const uint32_t nib = u[4] >> (32 - W);
#pragma unroll
  for (int i = 4; i > 0; i--) u[i] = (u[i] << W) | (u[i - 1] >> (32 - W));
  u[0] <<= W;
  const uint32_t dn = 0u - ((nib >> (W - 1)) ^ 1u);  // d < 0 (g < E)
  const uint32_t m = (nib ^ dn) & (E - 1);            // (|d| - 1) / 2: g - E, or E - 1 - g
  f_zero(e.X);
  f_zero(e.Y);
  f_zero(e.Z);
#pragma unroll
  for (int i = 0; i < (int)E; i++) {
    // m ^ i is 0 on a hit and 1 .. E - 1 otherwise: minus one is negative on a hit alone
    const uint32_t hit = bls_opaque((uint32_t)((int32_t)((m ^ (uint32_t)i) - 1u) >> 31));
#pragma unroll
    for (int w = 0; w < BN_LIMBS; w++) {
      e.X.v[w] |= tbl.get(i, w) & hit;
      e.Y.v[w] |= tbl.get(i, 9 + w) & hit;
      e.Z.v[w] |= tbl.get(i, 18 + w) & hit;
    }
  }
  fp z, ny;
  f_zero(z);
  f_sub_ct(ny, z, e.Y);
  f_sel_ct(e.Y, bls_opaque(dn ^ neg), ny, e.Y);
}

// out37 = be32(id) || compress(sk * H) for the signer record rec (bls_signer_record) and the public
// point H = g1_map(msg); tbl is this lane's table storage.
//
// Scheme.  T[m] = (2m + 1) H, m < 2^(W-1) (public, built here).  Each GLV half |k_h| < 2^128, made odd,
// is a chain of its own: 132 / W windows of W doublings and exactly one addition of +-T[.], as the row
// kernel's two waves, run one after the other in this lane (2 x 128 doublings after
// the first digit).
//
// Why no addition of a chain meets P = +-Q or infinity.  After a window the accumulator is s B with
// B = +-H and s the odd integer formed by the digits so far; the next addition is 2^W s B + d B with
// d odd, |d| < 2^W.  |2^W s +- d| is an integer in [1, 2^133) and r > 2^253, so 2^W s = +-d (mod r) would
// need 2^W |s| = |d| < 2^W with s odd, and 2^W s B itself is never infinity.  The table's additions are
// (2m - 1) H + 2 H, m < 2^(W-1).
// The halves could share their doublings (128 instead of 256): the accumulator is then
// s1 H + s2 phi(H), and an addition meets P = +-Q exactly when (2^W s1 -+ d, 2^W s2) or (2^W s1 + d1,
// 2^W s2 -+ d2) lies in the GLV lattice L = {(x, y): x + y lam = 0 mod r}.  L's shortest vector is
// v1 = (a1, b1) = (0x8100000000000001, -0x61818000000000020400000000000003), max norm 2^126.6, so
// nothing happens while 2^W |s| < 2^126 (all but the last two or three windows), but there such vectors
// exist for public, easily named keys: the split of sk = r - 1 is (-1, 0) + v1 + v2, whose final
// partial sums differ from the lattice vector v1 + v2 by single digits.  Ruling those out means
// knowing the split's rounding for every key; two chains need no such case list, so they are what
// runs, and the price (about 900 of 3,900 field multiplications per share) is paid.
//
// Closing corrections, all by selects: the odd fix (acc - B, which is infinity exactly when the half
// is 0: the incomplete addition then returns Z = 0 and the half is flagged), phi on the second half
// (X <- beta X), and the sum of the halves, which is the other half when one is flagged, the doubling
// when both are the same point ((k1, -k2) in L, e.g. sk = 2 a1) and the incomplete addition
// otherwise.  A half of 0 covers sk in {1, 2, 3, ..} (k2 = 0) and every other key whose split has a zero
// coordinate (this split gives lam itself full-size halves, not (0, 1): the cases depend on the
// rounding).  The sum is never infinity (sk != 0 mod r and H has order r).  The affine conversion is
// the constant-time Fermat inversion; the affine point is the public share.
template <int W, class Tbl>
BN_HD void bls_sign_lane(uint8_t* out37, const g1a& H, const uint32_t* rec, Tbl& tbl) {
  static_assert(BLS_SIGN_BITS % W == 0 && W >= 2 && W <= 4, "window");
  uint32_t hz, rz;
  g1j P, A[2];
  P.X = H.x;
  P.Y = H.y;
  f_one(P.Z);
  {
    g1j P2, t = P;
    g1_dbl_ct(P2, P);
    bls_tbl_put(tbl, 0, t);
    for (int m = 1; m < (1 << (W - 1)); m++) {
      g1j s;
      g1_add_ct(s, t, P2, hz, rz);
      t = s;
      bls_tbl_put(tbl, m, t);
    }
  }
  const uint32_t flags = rec[10];
  uint32_t inf[2];
  fp beta;
  {
    uint32_t bw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) bw[i] = BlsGlvConsts::BETA[i];
    f_from_words(beta, bw);
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
  for (int h = 0; h < 2; h++) {
    uint32_t u[5];
#pragma unroll
    for (int i = 0; i < 5; i++) u[i] = rec[5 * h + i];
    const uint32_t neg = bls_opaque(0u - ((flags >> h) & 1u));
    const uint32_t even = bls_opaque(0u - ((flags >> (2 + h)) & 1u));
    g1j acc, e, t;
    bls_sign_pick<W>(acc, u, neg, tbl);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int w = BLS_SIGN_BITS / W - 2; w >= 0; w--) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
      for (int d = 0; d < W; d++) {
        g1_dbl_ct(t, acc);
        acc = t;
      }
      bls_sign_pick<W>(e, u, neg, tbl);
      g1_add_ct(t, acc, e, hz, rz);
      acc = t;
    }
    // undo the odd fix: acc - B, B = +-H, kept where the half was even
    fp z, ny;
    f_zero(z);
    f_sub_ct(ny, z, P.Y);
    e = P;
    f_sel_ct(e.Y, neg, P.Y, ny);  // -B: -H unless the half is negative
    g1_add_ct(t, acc, e, hz, rz);
    g1_sel_ct(acc, even, t, acc);
    inf[h] = even & f_zero_mask_ct(t.Z);
    if (h == 1) f_mul(acc.X, acc.X, beta);  // phi (h is public)
    A[h] = acc;
  }
  g1j S, D, R;
  g1_add_ct(S, A[0], A[1], hz, rz);
  g1_dbl_ct(D, A[0]);
  g1_sel_ct(R, hz & rz, D, S);
  g1_sel_ct(R, inf[1], A[0], R);
  g1_sel_ct(R, inf[0], A[1], R);
  fp zi, zi2;
  fp_inv(zi, R.Z);
  g1a a;
  f_sqr(zi2, zi);
  f_mul(a.x, R.X, zi2);
  f_mul(zi2, zi2, zi);
  f_mul(a.y, R.Y, zi2);
  a.inf = false;
  const uint32_t id = rec[11];
  out37[0] = (uint8_t)(id >> 24);
  out37[1] = (uint8_t)(id >> 16);
  out37[2] = (uint8_t)(id >> 8);
  out37[3] = (uint8_t)id;
  g1_compress(out37 + 4, a);
}

// ------------------------------------------------------------------------------ launches (bls_sign_batch.hip)
#if defined(__HIPCC__)
// messages of one hash block: its lanes take them one at a time from an LDS counter
#define BLS_SIGN_HASH_CHUNK 256
// signatures per launch: bounds the scratch
#define BLS_SIGN_LAUNCH_MAX (1u << 20)
// Hash to G1.  Half of all x give a square, so a message needs 2 tries on average, but the unluckiest
// of 64 needs about 7: a wave that keeps one message per lane until all are done spends most of its
// rounds on a few lanes.  Here a block owns BLS_SIGN_HASH_CHUNK consecutive messages and its 64 lanes
// take them one at a time from an LDS counter: a lane whose message found its point takes the next
// pending one, and the wave runs rounds (one square root each) until nothing is pending.  Everything
// here is public (messages and their hash points), so the loop may branch.
// H is written [word][n] (18 words: x, y in Montgomery form), coalesced for the next kernel.
// STEAL = false is the plain loop (lane l keeps message l, l + 64, ..: a new message only when every
// lane is done), kept for the measurement in tests/hip/bls_sign_selftest.hip.
template <bool STEAL>
__global__ void __launch_bounds__(64) bls_sign_hash_kernel(const uint8_t* msg, const uint64_t* off, const uint32_t* len,
                                                           uint32_t fixed_len, uint32_t n, uint32_t* H,
                                                           uint32_t* rounds) {
  __shared__ uint32_t next;
  if (threadIdx.x == 0) next = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)BLS_SIGN_HASH_CHUNK;
  const uint32_t cnt = n - base < (uint32_t)BLS_SIGN_HASH_CHUNK ? n - base : (uint32_t)BLS_SIGN_HASH_CHUNK;
  bool have = false;
  uint32_t j = 0, r = 0, pass = 0;
  fp x, y;
  for (;;) {
    if (STEAL ? !have : !__any(have)) {
      const uint32_t t = STEAL ? atomicAdd(&next, 1u) : 64u * pass++ + threadIdx.x;
      if (t < cnt) {
        j = base + t;
        const uint8_t* m = off ? msg + off[j] : msg + (size_t)j * fixed_len;
        bls_map_x0(x, m, off ? len[j] : fixed_len);
        have = true;
      }
    }
    if (!__any(have)) break;
    if (have && bls_map_try(y, x)) {
#pragma unroll
      for (int w = 0; w < BN_LIMBS; w++) {
        H[(size_t)w * n + j] = x.v[w];
        H[(size_t)(BN_LIMBS + w) * n + j] = y.v[w];
      }
      have = false;
    }
    r++;
  }
  if (rounds && threadIdx.x == 0) rounds[blockIdx.x] = r;
}

// Table geometry: the 2^(W-1) Jacobian entries of a share in LDS, [entry][word][lane] (W = 3: 27 KB per
// wave, five waves fit a CU; W = 4: 54 KB, two waves), or (LDS = false) in global scratch
// [entry][word][n], coalesced and L2-resident.  The product runs <BLS_SIGN_W, true>; the others are built
// by the self-test harness for the measurement.
template <int W, bool LDS>
__global__ void __launch_bounds__(64) bls_sign_mul_kernel(uint32_t n, const uint32_t* rec, uint32_t nkeys,
                                                          const uint32_t* idx, const uint32_t* H, uint32_t* tbl,
                                                          uint8_t* out37) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  uint8_t* out = out37 + 37 * (size_t)i;
  const uint32_t s = idx ? idx[i] : 0u;  // public
  if (s >= nkeys) {
    for (int b = 0; b < 37; b++) out[b] = 0;
    return;
  }
  uint32_t r[BLS_SIGNER_WORDS];
#pragma unroll
  for (int w = 0; w < BLS_SIGNER_WORDS; w++) r[w] = rec[BLS_SIGNER_WORDS * (size_t)s + w];
  g1a h;
#pragma unroll
  for (int w = 0; w < BN_LIMBS; w++) {
    h.x.v[w] = H[(size_t)w * n + i];
    h.y.v[w] = H[(size_t)(BN_LIMBS + w) * n + i];
  }
  h.inf = false;
  __shared__ uint32_t lds[LDS ? BLS_SIGN_TBL_WORDS(W) * 64 : 1];
  BlsTblStrided t{LDS ? lds + threadIdx.x : tbl + i, LDS ? (size_t)64 : (size_t)n};
  bls_sign_lane<W>(out, h, r, t);
}

struct BlsSignBatch {
  size_t n;
  const uint32_t* rec;  // nkeys x BLS_SIGNER_WORDS
  uint32_t nkeys;
  const uint32_t* signer_idx;  // n, or nullptr = signer 0
  const uint8_t* msg;
  const uint64_t* off;  // n, or nullptr = fixed_len messages back to back
  const uint32_t* len;
  uint32_t fixed_len;
};
// scratch words for a batch of n: H (18 words) per signature of a launch
size_t cbft_bls_sign_scratch_words(size_t n);
// records from nkeys x 8 little-endian scalar words (each in [1, r)) and ids, one lane per signer
hipError_t cbft_bls_sign_launch_keys(const uint32_t* d_sk, const uint32_t* d_ids, uint32_t nkeys, uint32_t* d_rec,
                                     hipStream_t s);
// d_out37 = n x 37 bytes; a signer index >= nkeys gives 37 zero bytes.  d_rounds (nullable): the hash
// kernel's rounds per block, ceil(n / BLS_SIGN_HASH_CHUNK) words per launch chunk (measurement)
hipError_t cbft_bls_sign_launch(const BlsSignBatch& b, uint32_t* d_scratch, uint8_t* d_out37, uint32_t* d_rounds,
                                hipStream_t s);
#endif
