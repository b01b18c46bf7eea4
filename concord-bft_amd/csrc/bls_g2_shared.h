// Device code shared by the G2 key kernels (bls_keys.hip) and the batched multisig verification
// (bls_multisig_batch.hip): the normalisation of a key's Miller-loop lines, the tail of a key sum and
// the one-lane form of a row-parallel partial sum.
#pragma once
#include "bls_common.h"
#include "bls_kernels.h"
#include "bn254_g2wave.h"
#include "bn254_g2row.h"

// Normalised lines (lambda, mu: BN_LINE_WORDS words each, g2_precompute_lines_batch's values)
// from the wave's unnormalised (A, B, C) records in LDS, lambda_k = -B_k / A_k, mu_k = C_k / A_k,
// by Montgomery's trick over the A_k on row-parallel Fp: prefix products (one Fp2 product per
// step: one pass), one variable-time Fp2 inversion on every lane (public key material), the
// back-substitution (two Fp2 products per step: two passes), then the 140 lambda / mu products
// row-locally, four lines' coefficients at a time.  pre: BN_ATE_LINES x 18 words of LDS.
static __device__ __noinline__ void g2r_normalise_lines(uint32_t* out, const uint32_t* abc, uint32_t* pre) {
  using R2 = F2R<uint32_t>;
  const G2RowCtx<uint32_t, uint64_t> c(0u);
  uint32_t A[6], B[6], P[6];
  R2 acc = f2r_red(f2r_ld(abc), c);  // the records' coefficients are unreduced (< 50q)
  f2r_st_row0(pre, acc);
#pragma nounroll
  for (int k = 1; k < BN_ATE_LINES; k++) {
    const R2 a = f2r_red(f2r_ld(abc + k * BN_ABC_WORDS), c);
    f2r_mul_ops(A, B, 0, acc, a);
    r_prods<3>(P, A, B, c);
    f2r_mul_res(acc, P, 0, c);
    f2r_st_row0(pre + 18 * k, acc);
  }
  fp2 n;
  rf_to_fe(n.a, acc.a);
  rf_to_fe(n.b, acc.b);
  fp2_inv<true>(n, n);
  R2 inv = f2r_from(n);
#pragma nounroll
  for (int k = BN_ATE_LINES - 1; k >= 1; k--) {
    const R2 pk = f2r_ld(pre + 18 * (k - 1)), a = f2r_red(f2r_ld(abc + k * BN_ABC_WORDS), c);
    f2r_mul_ops(A, B, 0, inv, pk);  // 1 / A_k
    f2r_mul_ops(A, B, 3, inv, a);   // 1 / (A_0 .. A_{k-1})
    r_prods<6>(P, A, B, c);
    R2 ai;
    f2r_mul_res(ai, P, 0, c);
    f2r_mul_res(inv, P, 3, c);
    f2r_st_row0(pre + 18 * k, ai);
  }
  f2r_st_row0(pre, inv);
  const int row = (threadIdx.x & 63) >> 4;
#pragma nounroll
  for (int base = 0; base < 2 * BN_ATE_LINES; base += 4) {  // 140 = 35 x 4
    const int i = base + row, k = i >> 1, mu = i & 1;
    const R2 x = f2r_red(f2r_ld(abc + k * BN_ABC_WORDS + (mu ? 36 : 18)), c), y = f2r_ld(pre + 18 * k);
    const uint32_t p0 = c.mul(x.a, y.a), p1 = c.mul(x.b, y.b), p2 = c.mul(rf_add(x.a, x.b), rf_add(y.a, y.b));
    R2 r{c.red(c.sub(p0, p1)), c.red(c.sub(c.sub(p2, p0), p1))};
    const R2 nr = f2r_red(f2r_sub(R2{c.zero, c.zero}, r, c), c);
    r.a = mu ? r.a : nr.a;  // lambda = -B / A
    r.b = mu ? r.b : nr.b;
    f2r_st(out + (size_t)k * BN_LINE_WORDS + 18 * mu, r);
  }
}

// normalise and compress (out65) a summed key; bad = a selected key did not decode
static __device__ void g2_sum_tail(const g2j& acc, bool bad, uint8_t* ok, uint8_t* out65) {
  g2a s;
  g2_to_affine(s, acc);
  const bool good = !bad;
  if (good) {
    g2_compress(out65, s);
  } else {
    for (int q = 0; q < 65; q++) out65[q] = 0;
  }
  ok[0] = good && !s.inf ? 1 : 0;
}

using G2RCtx = G2RowCtx<uint32_t, uint64_t>;
// rows -> 54 one-lane words (< 2q: each coordinate through one Montgomery product with 1) + bad
__device__ __forceinline__ void g2r_part_store(uint32_t* o, const G2R<uint32_t>& p, bool inf, bool bad,
                                               const G2RCtx& c) {
  uint32_t A[6] = {p.X.a, p.X.b, p.Y.a, p.Y.b, p.Z.a, p.Z.b}, B[6], P[6];
  for (int i = 0; i < 6; i++) B[i] = c.one;
  r_prods<6>(P, A, B, c);
  for (int i = 0; i < 6; i++) rf_st9_row0(o + 9 * i, inf ? (i < 4 ? c.one : c.zero) : P[i]);
  if (__lane_id() == 0) o[54] = bad ? 1u : 0u;
}
__device__ __forceinline__ bool g2r_part_load(G2R<uint32_t>& p, const uint32_t* o, const G2RCtx& c) {
  p.X = f2r_ld(o);
  p.Y = f2r_ld(o + 18);
  p.Z = f2r_ld(o + 36);
  return c.zero4(p.Z);  // infinity
}
