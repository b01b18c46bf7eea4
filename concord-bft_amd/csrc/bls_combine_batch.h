// Batched BLS share combination on BN-P254 G1, one share per lane.
//
//   sigma_c = sum over the used shares j of certificate c of lambda_j sigma_j     (threshold)
//   sigma_c = sum over the used shares j of certificate c of sigma_j              (multisig)
//
// The lane-level routines below are one-lane BN_HD code (bn254_field.h), so the same source runs on
// gfx950 (bls_combine_batch.hip) and on the host (tests/cpp/bls_combine_shim.cpp).  Everything here
// is public data (shares, ids, coefficients, the combined signature): the code branches on it, reads
// one table entry per digit and skips zero digits.  bls_sign_batch.h is the constant-time counterpart
// for a secret scalar; only its GLV split (the same constants) and its table storage are used here.
#pragma once
#include "bls_ops.h"
#include "bls_sign_batch.h"

#define BLS_COMBINE_MAX_K 2048  // shares per certificate: ids are in [1, 2048] (IThresholdVerifier.h:36)
#define BLS_COMBINE_INV 2048    // entries of the inverse table (bls_kernels.h BLS_INV_TABLE)

// what stage 1 leaves per share
#define BLSC_UNUSED 0  // use[j] == 0: not decoded, not part of anything
#define BLSC_GOOD 1    // decoded, id in [1, 2048]
#define BLSC_BAD 2     // used, but undecodable or id out of range: closes its certificate
// per-share flags summed (OR) over a certificate by stage 4
#define BLSC_F_USED 1u
#define BLSC_F_BAD 2u  // a BLSC_BAD share, or a share whose id another used share repeats

// The complete Jacobian addition and the doubling as calls (g1_add / g1_dbl, bn254_pairing.h):
// g1_add decides infinity, P = Q (doubles) and P = -Q (infinity) by branches, which public data may take.
BN_HDN void blsc_add(g1j& r, const g1j& p, const g1j& q) { g1_add(r, p, q); }
BN_HDN void blsc_dbl(g1j& r, const g1j& p) { g1_dbl(r, p); }

// ------------------------------------------------------------------------------ stage 2: Lagrange
// lambda_i = prod_{j != i} id_j / (id_j - id_i) mod r over the BLSC_GOOD shares j of [lo, hi), as
// bls_lagrange_kernel forms it: id_j (Montgomery form, idm) into the numerator, inv[|id_j - id_i| - 1]
// into the inverted denominator, one sign flip per id_j < id_i; 2 (k - 1) products mod r.  The same
// walk finds a repeated id: returns true (lam8 is then not written).  With ids_only (multisig) only
// that check runs.  Share i itself must be BLSC_GOOD.
BN_HD bool blsc_lagrange_lane(uint32_t* lam8, const uint32_t* ids, const uint32_t* idm, const uint8_t* state,
                              uint32_t lo, uint32_t hi, uint32_t i, const uint32_t* inv, bool ids_only) {
  const uint32_t me = ids[i];
  fr num, den;
  f_one(num);
  f_one(den);
  uint32_t below = 0;
  for (uint32_t j = lo; j < hi; j++) {
    if (j == i || state[j] != BLSC_GOOD) continue;  // a BLSC_BAD id may be out of the table's range
    const uint32_t o = ids[j];
    if (o == me) return true;
    if (ids_only) continue;
    const uint32_t d = o > me ? o - me : me - o;  // 1 .. BLS_COMBINE_INV - 1
    fr t, iv;
#pragma unroll
    for (int q = 0; q < BN_LIMBS; q++) {
      t.v[q] = idm[BN_LIMBS * (size_t)j + q];
      iv.v[q] = inv[BN_LIMBS * (size_t)(d - 1) + q];
    }
    f_mul(num, num, t);
    f_mul(den, den, iv);
    below += o < me ? 1u : 0u;
  }
  if (ids_only) return false;
  f_mul(num, num, den);
  if (below & 1u) f_neg(num, num);
  f_to_words(lam8, num);
  return false;
}

// ------------------------------------------------------------------------------ stage 3: lambda * sigma
// Signed radix-8 digits of a half |k_h| < 2^128: u = |k_h| + 4 (8^0 + .. + 8^43) < 2^132, digit w is
// group w of u minus 4, in [-4, 3], and sum d_w 8^w = |k_h|.  u is kept shifted left by 28 bits so that
// the groups pop off the top of word 4, most significant first.
#define BLSC_W 3
#define BLSC_DIGITS 44
BN_HD void blsc_digits_init(uint32_t* u, const uint32_t* k5) {
  const uint32_t off[5] = {0x24924924u, 0x49249249u, 0x92492492u, 0x24924924u, 0x00000009u};
  uint32_t t[5];
  uint64_t cy = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    cy += (uint64_t)k5[i] + off[i];
    t[i] = (uint32_t)cy;
    cy >>= 32;
  }
#pragma unroll
  for (int i = 4; i >= 0; i--) u[i] = (t[i] << 28) | (i ? (t[i - 1] >> 4) : 0u);
}
BN_HD int blsc_digit_pop(uint32_t* u) {
  const int g = (int)(u[4] >> (32 - BLSC_W));
#pragma unroll
  for (int i = 4; i > 0; i--) u[i] = (u[i] << BLSC_W) | (u[i - 1] >> (32 - BLSC_W));
  u[0] <<= BLSC_W;
  return g - 4;
}

template <class Tbl>
BN_HD void blsc_tbl_get(g1j& p, const Tbl& tbl, int e) {
#pragma unroll
  for (int i = 0; i < BN_LIMBS; i++) {
    p.X.v[i] = tbl.get(e, i);
    p.Y.v[i] = tbl.get(e, 9 + i);
    p.Z.v[i] = tbl.get(e, 18 + i);
  }
}

// R = k * P for a public scalar k (8 LE words, < r) and a public point P; tbl is this lane's table
// storage (4 Jacobian entries: P, 2P, 3P, 4P).
//
// Scheme.  k = k1 + k2 lam (bls_glv_split_ct), phi(x, y) = (beta x, y) = lam (x, y).  Both halves run on
// ONE chain: 44 windows of three doublings, and per window one addition of +-T[|d| - 1] for the first
// half's digit and one of +-phi(T[|d| - 1]) for the second's, a zero digit adding nothing.  The
// accumulator is then s1 P + s2 phi(P), and for a P somebody chose (the shares are unverified on the
// optimistic path) nothing rules out that an addition meets its own operand, its negative or
// infinity: DESIGN.md §18.2 names the lattice vectors for which the merged chain does.  So every
// addition is the complete one (blsc_add): the three cases cost a branch that a wave takes only when
// one of its lanes is in it, and the halves share their 129 doublings, which two separate chains
// (§18.2's answer for a secret scalar, where a data-dependent branch is not allowed) would run twice.
template <class Tbl>
BN_HD void blsc_mul_lane(g1j& R, const g1a& P, const uint32_t* k, Tbl& tbl) {
  g1_set_inf(R);
  if (P.inf) return;
  uint32_t kk[2][5], n[2], u[2][5];
  bls_glv_split_ct(k, kk[0], kk[1], n[0], n[1]);
  blsc_digits_init(u[0], kk[0]);
  blsc_digits_init(u[1], kk[1]);
  {
    g1j t, t2, s;
    g1_from_affine(t, P);
    bls_tbl_put(tbl, 0, t);
    blsc_dbl(t2, t);
    bls_tbl_put(tbl, 1, t2);
    blsc_add(s, t2, t);
    bls_tbl_put(tbl, 2, s);
    blsc_dbl(s, t2);
    bls_tbl_put(tbl, 3, s);
  }
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
  for (int w = BLSC_DIGITS - 1; w >= 0; w--) {
    if (w != BLSC_DIGITS - 1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
      for (int d = 0; d < BLSC_W; d++) {
        g1j t;
        blsc_dbl(t, R);
        R = t;
      }
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int h = 0; h < 2; h++) {
      const int d = blsc_digit_pop(u[h]);
      if (d == 0) continue;
      g1j e, t;
      blsc_tbl_get(e, tbl, (d < 0 ? -d : d) - 1);
      if (h) f_mul(e.X, e.X, beta);
      if ((d < 0) != (n[h] != 0)) f_neg(e.Y, e.Y);
      blsc_add(t, R, e);
      R = t;
    }
  }
}

// ------------------------------------------------------------------------------ stage 4: the certificate
// The close of one certificate: the sum of its np partial sums (complete additions, so equal points
// double, opposite ones cancel and the sum goes on from infinity), one variable-time inversion,
// compression.  flags = the OR of its shares' flags: refused (status 0, 33 zero bytes) when a share
// was bad or nothing was used.  get(p, q) loads partial q.
template <class Get>
BN_HD void blsc_finish(uint8_t* out33, uint8_t* status, uint32_t flags, uint32_t np, Get get) {
  if ((flags & BLSC_F_BAD) || !(flags & BLSC_F_USED)) {
    for (int b = 0; b < 33; b++) out33[b] = 0;
    *status = 0;
    return;
  }
  g1j acc;
  g1_set_inf(acc);
  for (uint32_t q = 0; q < np; q++) {
    g1j o, t;
    get(o, q);
    blsc_add(t, acc, o);
    acc = t;
  }
  g1a a;
  g1_to_affine<true>(a, acc);
  g1_compress(out33, a);
  *status = 1;
}

// ------------------------------------------------------------------------------ launches (bls_combine_batch.hip)
#if defined(__HIPCC__)
// shares per launch sequence: bounds the scratch (cbft_bls_combine_batch_scratch_bytes)
#define BLS_COMBINE_LAUNCH_MAX (1u << 20)
// shares per call
#define BLS_COMBINE_BATCH_MAX (1u << 26)

struct BlsCombineBatch {
  uint32_t n;             // shares of this launch sequence (<= BLS_COMBINE_LAUNCH_MAX)
  uint32_t m;             // certificates
  const uint8_t* shares;  // n x 37
  const uint8_t* use;     // n, or nullptr = every share is used
  const uint32_t* off;    // m + 1 share offsets (off[0] = 0, off[m] = n), or nullptr = k shares each
  uint32_t k;
  int multisig;
  const uint32_t* inv;    // bls_inv_table_kernel's table (threshold only)
  uint8_t* out33;         // m x 33
  uint8_t* status;        // m
};
// bytes of scratch for a launch sequence over n shares
size_t cbft_bls_combine_batch_scratch_bytes(size_t n);
// ev (nullable): five events recorded before stage 1 and after each of the four stages (measurement)
hipError_t cbft_bls_combine_batch_launch(const BlsCombineBatch& b, void* d_scratch, hipStream_t s,
                                         hipEvent_t* ev = nullptr);
#endif
