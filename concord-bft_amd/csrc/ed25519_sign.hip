// Batched Ed25519 signing for gfx950 (MI355X), byte-exact with OpenSSL (RFC 8032 §5.1.6).
//
//   per signer, at load:  (h0 || h1) = SHA-512(seed);  a = clamp(h0);  prefix = h1;  A = encode([a]B)
//   per signature:        r = SHA-512(prefix || M) mod L;  R = encode([r]B);
//                         k = SHA-512(R || A || M) mod L;  S = (r + k a) mod L;  out = R || S
//
// One signature per lane, three launches so that each phase gets its own register budget (as the
// verify's K1..K4): the two hashes want the SHA-512 state and schedule in registers,
// the point kernel a p3 accumulator, the selected table entry and the inversion chain.
//
//   S1 ed25519_sign_nonce_kernel   r = SHA-512(prefix || M) mod L          -> r[8][n] (scratch)
//   S2 ed25519_sign_point_kernel   R = encode([r]B)                        -> sig[i][0..32)
//   S3 ed25519_sign_finish_kernel  k = SHA-512(R || A || M) mod L, S       -> sig[i][32..64), r cleared
//
// Secret independence: the signer index, the message length and the message bytes are public and
// decide addresses and the SHA-512 block count; a, prefix and r only ever flow through the
// arithmetic and selects of ed25519_sign.h, sha512.h, sc25519.h and fe25519.h (DESIGN.md §14
// lists each helper).  An out-of-range signer index (public) yields 64 zero bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CBFT_SIGN_DEVICE_HELPERS
#include "ed25519_sign.h"

__device__ __forceinline__ uint32_t sign_signer(const Ed25519SignBatch& b, size_t i, bool& valid) {
  const uint32_t idx = b.signer_idx ? b.signer_idx[i] : 0u;
  valid = idx < b.nkeys;
  return valid ? idx : 0u;
}
__device__ __forceinline__ const uint8_t* sign_msg(const Ed25519SignBatch& b, size_t i, uint32_t& len) {
  if (b.msg_off) {
    len = b.msg_len[i];
    return b.msg + b.msg_off[i];
  }
  len = b.fixed_len;
  return b.msg + i * (size_t)b.fixed_len;
}

// Table of B: one lane per comb position.
__global__ void __launch_bounds__(64) ed25519_sign_table_kernel(uint32_t* tbl) {
  if (blockIdx.x != 0 || threadIdx.x >= CBFT_SIGN_NPOS) return;
  sign_table_build_lane(tbl, (int)threadIdx.x);
}

// Signer records from seeds, one lane per signer.
__global__ void __launch_bounds__(CBFT_SIGN_BLOCK) ed25519_sign_keys_kernel(const uint8_t* seed, uint32_t nkeys,
                                                                            const uint32_t* __restrict__ tbl,
                                                                            uint32_t* signers) {
  const uint32_t i = blockIdx.x * CBFT_SIGN_BLOCK + threadIdx.x;
  if (i >= nkeys) return;
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(seed) + (size_t)i * 8;
  uint32_t s[8], h[16];
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = sw[k];
  sha512_prefix_m(h, s, nullptr, 0u);  // SHA-512(seed)
  h[0] &= 0xfffffff8u;
  h[7] = (h[7] & 0x3fffffffu) | 0x40000000u;
  uint32_t* rec = signers + (size_t)i * CBFT_SIGNER_WORDS;
#pragma unroll
  for (int k = 0; k < 16; k++) rec[k] = h[k];  // a | prefix
  // [a]B = [a mod L]B: the comb's recoding needs a scalar below 2^254.9
  uint32_t x[16], am[8], A[8];
#pragma unroll
  for (int k = 0; k < 16; k++) x[k] = k < 8 ? h[k] : 0u;
  sc_reduce512(am, x);
  sign_base_mul_encode(A, am, tbl);
#pragma unroll
  for (int k = 0; k < 8; k++) rec[16 + k] = A[k];
}

__global__ void __launch_bounds__(CBFT_SIGN_BLOCK) ed25519_sign_nonce_kernel(const Ed25519SignBatch b, uint32_t* r_soa) {
  const size_t i = (size_t)blockIdx.x * CBFT_SIGN_BLOCK + threadIdx.x;
  if (i >= b.n) return;
  bool valid;
  const uint32_t idx = sign_signer(b, i, valid);
  const uint32_t* rec = b.signers + (size_t)idx * CBFT_SIGNER_WORDS;
  uint32_t prefix[8], h[16], r[8];
#pragma unroll
  for (int k = 0; k < 8; k++) prefix[k] = rec[8 + k];
  uint32_t len;
  const uint8_t* m = sign_msg(b, i, len);
  sha512_prefix_m(h, prefix, m, len);
  sc_reduce512(r, h);
#pragma unroll
  for (int k = 0; k < 8; k++) r_soa[k * b.n + i] = r[k];
}

__global__ void __launch_bounds__(CBFT_SIGN_BLOCK) ed25519_sign_point_kernel(const Ed25519SignBatch b,
                                                                             const uint32_t* __restrict__ tbl,
                                                                             const uint32_t* r_soa, uint32_t* sig) {
  const size_t i = (size_t)blockIdx.x * CBFT_SIGN_BLOCK + threadIdx.x;
  if (i >= b.n) return;
  bool valid;
  (void)sign_signer(b, i, valid);
  uint32_t r[8], R[8];
#pragma unroll
  for (int k = 0; k < 8; k++) r[k] = r_soa[k * b.n + i];
  sign_base_mul_encode(R, r, tbl);
#pragma unroll
  for (int k = 0; k < 8; k++) sig[i * 16 + k] = valid ? R[k] : 0u;
}

__global__ void __launch_bounds__(CBFT_SIGN_BLOCK) ed25519_sign_finish_kernel(const Ed25519SignBatch b, uint32_t* r_soa,
                                                                              uint32_t* sig) {
  const size_t i = (size_t)blockIdx.x * CBFT_SIGN_BLOCK + threadIdx.x;
  if (i >= b.n) return;
  bool valid;
  const uint32_t idx = sign_signer(b, i, valid);
  const uint32_t* rec = b.signers + (size_t)idx * CBFT_SIGNER_WORDS;
  uint32_t R[8], A[8], a[8], r[8], h[16], k8[8], S[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    R[k] = sig[i * 16 + k];
    A[k] = rec[16 + k];
    a[k] = rec[k];
    r[k] = r_soa[k * b.n + i];
  }
  uint32_t len;
  const uint8_t* m = sign_msg(b, i, len);
  sha512_ram(h, R, A, m, len);
  sc_reduce512(k8, h);
  sc_muladd(S, r, k8, a);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    sig[i * 16 + 8 + k] = valid ? S[k] : 0u;
    r_soa[k * b.n + i] = 0u;  // the nonce is secret: it does not outlive its batch
  }
}

hipError_t cbft_ed25519_sign_build_table(uint32_t* d_tbl, hipStream_t stream) {
  hipLaunchKernelGGL(ed25519_sign_table_kernel, dim3(1), dim3(64), 0, stream, d_tbl);
  return hipGetLastError();
}

hipError_t cbft_ed25519_sign_launch_keys(const uint8_t* d_seed, uint32_t nkeys, const uint32_t* d_tbl,
                                         uint32_t* d_signers, hipStream_t stream) {
  if (nkeys == 0) return hipSuccess;
  const unsigned blocks = (nkeys + CBFT_SIGN_BLOCK - 1) / CBFT_SIGN_BLOCK;
  hipLaunchKernelGGL(ed25519_sign_keys_kernel, dim3(blocks), dim3(CBFT_SIGN_BLOCK), 0, stream, d_seed, nkeys, d_tbl,
                     d_signers);
  return hipGetLastError();
}

hipError_t cbft_ed25519_sign_launch(const Ed25519SignBatch& b, const uint32_t* d_tbl, uint32_t* d_scratch,
                                    uint8_t* d_sig, hipStream_t stream) {
  if (b.n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((b.n + CBFT_SIGN_BLOCK - 1) / CBFT_SIGN_BLOCK);
  uint32_t* sig = reinterpret_cast<uint32_t*>(d_sig);
  hipLaunchKernelGGL(ed25519_sign_nonce_kernel, dim3(blocks), dim3(CBFT_SIGN_BLOCK), 0, stream, b, d_scratch);
  hipLaunchKernelGGL(ed25519_sign_point_kernel, dim3(blocks), dim3(CBFT_SIGN_BLOCK), 0, stream, b, d_tbl, d_scratch,
                     sig);
  hipLaunchKernelGGL(ed25519_sign_finish_kernel, dim3(blocks), dim3(CBFT_SIGN_BLOCK), 0, stream, b, d_scratch, sig);
  return hipGetLastError();
}
