// Test-only device harness of the batched BLS key derivation (csrc/bls_keygen_batch.h), for the
// measurement of DESIGN.md §26 (tools/bls_keygen_bench.py): the product kernel (one key per lane) beside
// the rejected geometry, the lone call's row-parallel comb (bls_keys.hip bls_pubkey_row_kernel) launched
// over a grid with one key per 64-lane block, each timed with events around it on the same scalars.
// Not part of the product library.
#include <hip/hip_runtime.h>

#include "bls_common.h"
#include "bn254_g2wave.h"
#include "bn254_g2row.h"
#include "bls_kernels.h"
#include "../../concord-bft_amd/csrc/bls_keygen_batch.hip"

#define ST_HIP(x)                    \
  do {                               \
    hipError_t e_ = (x);             \
    if (e_ != hipSuccess) return -(int)e_ - 1000; \
  } while (0)

// bls_pubkey_row_kernel with the key taken from the block index: sk = n x 8 little-endian words, each
// in [1, r).  The same recoding, picks and blinded inversion, one key per block.
__global__ void __launch_bounds__(64) st_pubkey_row_grid_kernel(const uint32_t* tbl, const uint32_t* sk, uint8_t* out65) {
  using Ctx = G2RowCtx<uint32_t, uint64_t>;
  const Ctx c(0u);
  sk += 8 * (size_t)blockIdx.x;
  out65 += 65 * (size_t)blockIdx.x;
  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = sk[i];
  const uint32_t even = (k[0] & 1u) ^ 1u, emask = 0u - even;
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
  {
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
  auto pick = [&](int j, F2R<uint32_t>& qx, F2R<uint32_t>& qy) {
    const uint32_t nib = (u[j >> 3] >> (4 * (j & 7))) & 15u;
    const uint32_t dn = nib < 8u ? 1u : 0u;
    const uint32_t m = dn ? 7u - nib : nib - 8u;
    const uint32_t* base = tbl + (size_t)j * BLS_KG_ENT * BLS_KG_WORDS;
    qx = f2r_ld(base);
    qy = f2r_ld(base + 18);
#pragma unroll
    for (int e = 1; e < BLS_KG_ENT; e++) {
      const F2R<uint32_t> ex = f2r_ld(base + e * BLS_KG_WORDS), ey = f2r_ld(base + e * BLS_KG_WORDS + 18);
      const bool hit = m == (uint32_t)e;
      qx.a = rf_sel(hit, ex.a, qx.a);
      qx.b = rf_sel(hit, ex.b, qx.b);
      qy.a = rf_sel(hit, ey.a, qy.a);
      qy.b = rf_sel(hit, ey.b, qy.b);
    }
    const F2R<uint32_t> ny{c.sub(c.zero, qy.a), c.sub(c.zero, qy.b)};
    qy.a = c.red(rf_sel(dn != 0u, ny.a, qy.a));
    qy.b = c.red(rf_sel(dn != 0u, ny.b, qy.b));
  };
  G2R<uint32_t> acc;
  {
    F2R<uint32_t> qx, qy;
    pick(0, qx, qy);
    acc.X = qx;
    acc.Y = qy;
    acc.Z = F2R<uint32_t>{c.one, c.zero};
  }
#pragma nounroll
  for (int j = 1; j < BLS_KG_POS; j++) {
    F2R<uint32_t> qx, qy;
    pick(j, qx, qy);
    bool same_y;
    g2r_madd<false>((F2R<uint32_t>*)nullptr, acc, qx, qy, c, same_y);
  }
  {
    const F2R<uint32_t> ny{c.red(c.sub(c.zero, acc.Y.a)), c.red(c.sub(c.zero, acc.Y.b))};
    acc.Y.a = rf_sel(even != 0u, ny.a, acc.Y.a);
    acc.Y.b = rf_sel(even != 0u, ny.b, acc.Y.b);
  }
  g2j J;
  rf_to_fe(J.X.a, acc.X.a);
  rf_to_fe(J.X.b, acc.X.b);
  rf_to_fe(J.Y.a, acc.Y.a);
  rf_to_fe(J.Y.b, acc.Y.b);
  rf_to_fe(J.Z.a, acc.Z.a);
  rf_to_fe(J.Z.b, acc.Z.b);
  uint32_t bw[8];
  {
    uint32_t hs[8];
    sha256_key_msg(hs, k, 0x5c, nullptr, 0);
    for (int i = 0; i < 8; i++) bw[i] = sha256_bswap(hs[i]);
    bw[7] &= 0x1fffffffu;
    bw[0] |= (bw[0] | bw[1] | bw[2] | bw[3] | bw[4] | bw[5] | bw[6] | bw[7]) == 0u ? 1u : 0u;
  }
  fp b;
  f_from_words(b, bw);
  fp2 zb, zi, zi2;
  g2a a;
  fp2_mul_fp(zb, J.Z, b);
  fp2_inv<true>(zi, zb);
  fp2_mul_fp(zi, zi, b);
  fp2_sqr(zi2, zi);
  fp2_mul(a.x, J.X, zi2);
  fp2_mul(zi2, zi2, zi);
  fp2_mul(a.y, J.Y, zi2);
  a.inf = false;
  if (__lane_id() == 0) g2_compress(out65, a);
}

template <class T>
struct Dev {
  T* p = nullptr;
  ~Dev() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t n) { return hipMalloc(&p, (n ? n : 1) * sizeof(T)); }
};

extern "C" {

// n scalars (32 bytes big-endian each, every one in [1, r)), n <= BLS_KEYGEN_LAUNCH_MAX, through both
// geometries `reps` times: out_lane65 / out_row65 = n x 65 bytes of the last repetition, ms_lane / ms_row
// = reps event times each.  The comb table is built by the product's kernel first (untimed).
int bls_keygen_selftest_geometries(const uint8_t* sk32, uint32_t n, int reps, uint8_t* out_lane65, uint8_t* out_row65,
                                   float* ms_lane, float* ms_row) {
  if (n == 0 || n > BLS_KEYGEN_LAUNCH_MAX || reps < 1) return -1;
  Dev<uint32_t> tbl, skw;
  Dev<uint8_t> skb, o1, o2, ok;
  ST_HIP(tbl.alloc(cbft_bls_pub_table_words()));
  ST_HIP(skw.alloc(8 * (size_t)n));
  ST_HIP(skb.alloc(32 * (size_t)n));
  ST_HIP(o1.alloc(65 * (size_t)n));
  ST_HIP(o2.alloc(65 * (size_t)n));
  ST_HIP(ok.alloc(n));
  {
    uint32_t* w = new uint32_t[8 * (size_t)n];
    for (uint32_t i = 0; i < n; i++) be32_to_words(w + 8 * (size_t)i, sk32 + 32 * (size_t)i);
    const hipError_t e = hipMemcpy(skw.p, w, 32 * (size_t)n, hipMemcpyHostToDevice);
    delete[] w;
    ST_HIP(e);
  }
  ST_HIP(hipMemcpy(skb.p, sk32, 32 * (size_t)n, hipMemcpyHostToDevice));
  ST_HIP(cbft_bls_launch_pub_table(tbl.p, 0));
  ST_HIP(hipDeviceSynchronize());
  hipEvent_t ev[2];
  ST_HIP(hipEventCreate(&ev[0]));
  ST_HIP(hipEventCreate(&ev[1]));
  int rc = 0;
  for (int r = 0; r < reps && rc == 0; r++) {
    hipError_t e = hipEventRecord(ev[0], 0);
    if (e == hipSuccess) e = cbft_bls_keygen_launch(tbl.p, skb.p, nullptr, n, o1.p, ok.p, 0);
    if (e == hipSuccess) e = hipEventRecord(ev[1], 0);
    if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms_lane[r], ev[0], ev[1]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], 0);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(st_pubkey_row_grid_kernel, dim3(n), dim3(64), 0, 0, (const uint32_t*)tbl.p, (const uint32_t*)skw.p,
                         o2.p);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev[1], 0);
    if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms_row[r], ev[0], ev[1]);
    if (e != hipSuccess) rc = -(int)e - 1000;
  }
  if (rc == 0 && hipMemcpy(out_lane65, o1.p, 65 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) rc = -2;
  if (rc == 0 && hipMemcpy(out_row65, o2.p, 65 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) rc = -2;
  (void)hipMemset(skw.p, 0, 32 * (size_t)n);
  (void)hipMemset(skb.p, 0, 32 * (size_t)n);
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  return rc;
}

}  // extern "C"
