// Batched, constant-time BLS share signing on BN-P254 G1: the kernels around the
// lane routines of bls_sign_batch.h.
//
//   bls_sign_keys_kernel  one lane per signer: GLV split, odd fix and digit recoding -> the record
//   bls_sign_hash_kernel  H = g1_map(msg): try-and-increment scheduled per block (public data)
//   bls_sign_mul_kernel   one lane per share: table of H's odd multiples (LDS), the two GLV chains, the
//                         closing corrections, Fermat inversion, compression
#include "bls_sign_batch.h"

__global__ void __launch_bounds__(64) bls_sign_keys_kernel(const uint32_t* sk, const uint32_t* ids, uint32_t nkeys,
                                                           uint32_t* rec) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= nkeys) return;
  uint32_t k[8], r[BLS_SIGNER_WORDS];
#pragma unroll
  for (int w = 0; w < 8; w++) k[w] = sk[8 * (size_t)i + w];
  bls_signer_record(r, k, ids[i]);
#pragma unroll
  for (int w = 0; w < BLS_SIGNER_WORDS; w++) rec[BLS_SIGNER_WORDS * (size_t)i + w] = r[w];
}

size_t cbft_bls_sign_scratch_words(size_t n) {
  const size_t m = n < BLS_SIGN_LAUNCH_MAX ? n : BLS_SIGN_LAUNCH_MAX;
  return m * (2 * BN_LIMBS);
}

hipError_t cbft_bls_sign_launch_keys(const uint32_t* d_sk, const uint32_t* d_ids, uint32_t nkeys, uint32_t* d_rec,
                                     hipStream_t s) {
  hipLaunchKernelGGL(bls_sign_keys_kernel, dim3((nkeys + 63) / 64), dim3(64), 0, s, d_sk, d_ids, nkeys, d_rec);
  return hipGetLastError();
}

hipError_t cbft_bls_sign_launch(const BlsSignBatch& b, uint32_t* d_scratch, uint8_t* d_out37, uint32_t* d_rounds,
                                hipStream_t s) {
  for (size_t at = 0; at < b.n; at += BLS_SIGN_LAUNCH_MAX) {
    const uint32_t m = (uint32_t)(b.n - at < BLS_SIGN_LAUNCH_MAX ? b.n - at : BLS_SIGN_LAUNCH_MAX);
    uint32_t* d_H = d_scratch;
    const uint32_t hb = (m + BLS_SIGN_HASH_CHUNK - 1) / BLS_SIGN_HASH_CHUNK;
    hipLaunchKernelGGL(bls_sign_hash_kernel<true>, dim3(hb), dim3(64), 0, s,
                       b.off ? b.msg : b.msg + at * b.fixed_len, b.off ? b.off + at : nullptr,
                       b.len ? b.len + at : nullptr, b.fixed_len, m, d_H, d_rounds);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((bls_sign_mul_kernel<BLS_SIGN_W, true>), dim3((m + 63) / 64), dim3(64), 0, s, m, b.rec, b.nkeys,
                       b.signer_idx ? b.signer_idx + at : nullptr, d_H, (uint32_t*)nullptr, d_out37 + 37 * at);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (d_rounds) d_rounds += hb;
  }
  return hipSuccess;
}
