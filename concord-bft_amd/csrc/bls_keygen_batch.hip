// Batched BLS key derivation and Shamir dealing on gfx950: the kernels around the lane routines of
// bls_keygen_batch.h.  One key, one coefficient or one share per lane.
#include "bls_keygen_batch.h"

static_assert(BLS_KG_POS == 64 && BLS_KG_ENT == 8 && BLS_KG_WORDS == 36, "the comb of bls_keys.hip");

// vk_i = (sk_i mod r) g2.  The lane index and n are public; a lane past n leaves before it reads.
__global__ void __launch_bounds__(64) bls_keygen_mul_kernel(const uint32_t* __restrict__ tbl,
                                                            const uint8_t* __restrict__ sk32,
                                                            const uint32_t* __restrict__ skw, uint32_t n,
                                                            uint8_t* __restrict__ out65, uint8_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  uint32_t k[8];
  if (sk32) {  // which form the caller gave is public
    be32_to_words(k, sk32 + 32 * (size_t)i);
  } else {
#pragma unroll
    for (int w = 0; w < 8; w++) k[w] = skw[8 * (size_t)i + w];
  }
  uint8_t good;
  bls_keygen_lane(out65 + 65 * (size_t)i, &good, k, tbl);
  if (ok) ok[i] = good;
}

// coefficient j -> Montgomery form mont[j][limb]; lane 0 also leaves c_0 mod r as share slot 0
__global__ void __launch_bounds__(64) bls_keygen_coeff_kernel(const uint8_t* __restrict__ coeff32, uint32_t k,
                                                              uint32_t* __restrict__ mont, uint8_t* __restrict__ sk32) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  if (j >= k) return;
  fr c;
  bls_kg_coeff(c, coeff32 + 32 * (size_t)j);
#pragma unroll
  for (int i = 0; i < BN_LIMBS; i++) mont[(size_t)j * BN_LIMBS + i] = c.v[i];
  if (j == 0) {
    uint32_t w[8];
    bls_kg_fr_words(w, c);
    words_to_be32(sk32, w);
  }
}

// share id = lane + 1: Horner over the k coefficients (every lane reads the same coefficient: uniform
// addresses that depend on the public j alone)
__global__ void __launch_bounds__(64) bls_keygen_eval_kernel(const uint32_t* __restrict__ mont, uint32_t k, uint32_t n,
                                                             uint8_t* __restrict__ sk32) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  bls_kg_eval_lane(sk32 + 32 * (size_t)(i + 1), mont, BN_LIMBS, k, i + 1);
}

hipError_t cbft_bls_keygen_launch(const uint32_t* d_tbl, const uint8_t* d_sk32, const uint32_t* d_skw, uint32_t n,
                                  uint8_t* d_out65, uint8_t* d_ok, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (n > BLS_KEYGEN_LAUNCH_MAX || (!d_sk32 && !d_skw)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bls_keygen_mul_kernel, dim3((n + 63) / 64), dim3(64), 0, s, d_tbl, d_sk32, d_skw, n, d_out65,
                     d_ok);
  return hipGetLastError();
}

hipError_t cbft_bls_keygen_launch_deal(const uint8_t* d_coeff32, uint32_t k, uint32_t n, uint32_t* d_mont,
                                       uint8_t* d_sk32, hipStream_t s) {
  if (k == 0 || n == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bls_keygen_coeff_kernel, dim3((k + 63) / 64), dim3(64), 0, s, d_coeff32, k, d_mont, d_sk32);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bls_keygen_eval_kernel, dim3((n + 63) / 64), dim3(64), 0, s, (const uint32_t*)d_mont, k, n, d_sk32);
  return hipGetLastError();
}
