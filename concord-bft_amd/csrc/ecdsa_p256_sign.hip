// Batched deterministic ECDSA P-256 / SHA-256 signing for gfx950 (MI355X): ecdsa_p256_sign.h's lane
// routines, one signer / one message per lane.  The split is ecdsa_sign.hip's:
//
//   ecdsa_p256_sign_table_kernel   G's comb table (public), one lane per position, once per context
//   ecdsa_p256_sign_keys_kernel    x -> record x | Q = x G | validity, one signer per lane
//   per batch:
//   S1 ecdsa_p256_sign_nonce_kernel   h1 = SHA-256(m), RFC 6979 nonce              -> k, h1, state (scratch)
//   S2 ecdsa_p256_sign_point_kernel   R = k G, r, k^-1, s -> r || s; clears k; r = 0 or s = 0 -> state REDO
//   S3 ecdsa_p256_sign_redo_kernel    lanes in state REDO (probability about 2^-255 each) sign again with
//                                     the whole lane routine, which passes over the refused candidates
//
// k crosses one launch boundary in the context's scratch (k[8][n], structure of arrays) and is
// zeroed by S2, its only reader.  h1 and the state word are public.
//
// Secret independence: the signer index, its validity, the message bytes and lengths are public and
// decide addresses, the SHA-256 block count and whether a lane signs at all; x, k, K, V, k^-1 and
// the point's coordinates flow through ecdsa_p256_sign.h's arithmetic and selects alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ecdsa_p256_sign.h"

#define P2S_BLOCK 64

__global__ void __launch_bounds__(128) ecdsa_p256_sign_table_kernel(uint32_t* tbl) {
  if (blockIdx.x != 0 || threadIdx.x >= ECDSAS_TABLE_LANES) return;
  p2s_table_lane(tbl, (int)threadIdx.x);
}

__global__ void __launch_bounds__(P2S_BLOCK) ecdsa_p256_sign_keys_kernel(const uint8_t* priv, uint32_t nkeys,
                                                                         const uint32_t* __restrict__ tbl,
                                                                         uint32_t* signers) {
  const uint32_t i = blockIdx.x * P2S_BLOCK + threadIdx.x;
  if (i >= nkeys) return;
  p2s_signer_lane(signers + (size_t)i * ECDSAS_WORDS, priv + (size_t)i * ECDSAS_PRIV_BYTES, tbl);
}

// state word of a lane between the launches
#define P2S_ST_NONE 0u   // no signature: 64 zero bytes (no such signer, or its key was refused at load)
#define P2S_ST_READY 1u  // k and h1 are in the scratch
#define P2S_ST_REDO 2u   // r = 0 or s = 0 under the first nonce

__device__ __forceinline__ const uint32_t* p2s_record(const EcdsaSignBatch& b, size_t i, bool& usable) {
  const uint32_t idx = b.signer_idx ? b.signer_idx[i] : 0u;
  const uint32_t* rec = b.signers + (size_t)(idx < b.nkeys ? idx : 0u) * ECDSAS_WORDS;
  usable = idx < b.nkeys && rec[ECDSAS_OK] != 0u;  // public
  return rec;
}

__global__ void __launch_bounds__(P2S_BLOCK) ecdsa_p256_sign_nonce_kernel(const EcdsaSignBatch b, uint32_t* scratch) {
  const size_t i = (size_t)blockIdx.x * P2S_BLOCK + threadIdx.x;
  if (i >= b.n) return;
  bool usable;
  const uint32_t* rec = p2s_record(b, i, usable);
  uint32_t* state = scratch + 16 * b.n;
  if (!usable) {
#pragma unroll
    for (int k = 0; k < 16; k++) scratch[k * b.n + i] = 0u;
    state[i] = P2S_ST_NONE;
    return;
  }
  const uint8_t* m;
  uint32_t len;
  if (b.msg_off) {
    len = b.msg_len[i];
    m = b.msg + b.msg_off[i];
  } else {
    len = b.fixed_len;
    m = b.msg + i * (size_t)b.fixed_len;
  }
  const uint32_t N[8] = P2_N_LIMBS;
  uint32_t h1[8], x[8], kk[8];
  ecdsa_sha256(h1, m, len);
#pragma unroll
  for (int k = 0; k < 8; k++) x[k] = rec[k];
  (void)ecdsas_nonce(kk, x, h1, N);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    scratch[k * b.n + i] = kk[k];
    scratch[(8 + k) * b.n + i] = h1[k];
  }
  state[i] = P2S_ST_READY;
}

__global__ void __launch_bounds__(P2S_BLOCK) ecdsa_p256_sign_point_kernel(const EcdsaSignBatch b,
                                                                          const uint32_t* __restrict__ tbl,
                                                                          uint32_t* scratch, uint32_t* sig) {
  const size_t i = (size_t)blockIdx.x * P2S_BLOCK + threadIdx.x;
  if (i >= b.n) return;
  uint32_t* out = sig + i * 16;
  uint32_t* state = scratch + 16 * b.n;
  if (state[i] != P2S_ST_READY) {
#pragma unroll
    for (int k = 0; k < 16; k++) out[k] = 0u;
    return;
  }
  bool usable;
  const uint32_t* rec = p2s_record(b, i, usable);
  uint32_t x[8], kk[8], z[8], s16[16];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    x[k] = rec[k];
    kk[k] = scratch[k * b.n + i];
    z[k] = scratch[(15 - k) * b.n + i];  // h1 as an integer's limbs
    scratch[k * b.n + i] = 0u;           // the nonce is secret: it does not outlive its reader
  }
  P2Sc e, r, s;
  p2_sc_reduce256(e, z);
  const uint32_t ok = p2s_sign_with_k(r, s, x, e, kk, tbl);
  p2s_put_sig(s16, r, s);
#pragma unroll
  for (int k = 0; k < 16; k++) out[k] = s16[k] & ok;
  state[i] = ok ? P2S_ST_NONE : P2S_ST_REDO;
}

__global__ void __launch_bounds__(P2S_BLOCK) ecdsa_p256_sign_redo_kernel(const EcdsaSignBatch b,
                                                                         const uint32_t* __restrict__ tbl,
                                                                         uint32_t* scratch, uint32_t* sig) {
  const size_t i = (size_t)blockIdx.x * P2S_BLOCK + threadIdx.x;
  if (i >= b.n) return;
  uint32_t* state = scratch + 16 * b.n;
  if (state[i] != P2S_ST_REDO) return;
  bool usable;
  const uint32_t* rec = p2s_record(b, i, usable);
  uint32_t h1[8], x[8], s16[16];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    x[k] = rec[k];
    h1[k] = scratch[(8 + k) * b.n + i];
  }
  p2s_sign_lane(s16, x, h1, tbl);
#pragma unroll
  for (int k = 0; k < 16; k++) sig[i * 16 + k] = s16[k];
  state[i] = P2S_ST_NONE;
}

hipError_t cbft_ecdsa_p256_sign_build_table(uint32_t* d_tbl, hipStream_t stream) {
  hipLaunchKernelGGL(ecdsa_p256_sign_table_kernel, dim3(1), dim3(128), 0, stream, d_tbl);
  return hipGetLastError();
}

hipError_t cbft_ecdsa_p256_sign_launch_keys(const uint8_t* d_priv, uint32_t nkeys, const uint32_t* d_tbl,
                                            uint32_t* d_signers, hipStream_t stream) {
  if (nkeys == 0) return hipSuccess;
  const unsigned blocks = (nkeys + P2S_BLOCK - 1) / P2S_BLOCK;
  hipLaunchKernelGGL(ecdsa_p256_sign_keys_kernel, dim3(blocks), dim3(P2S_BLOCK), 0, stream, d_priv, nkeys, d_tbl, d_signers);
  return hipGetLastError();
}

hipError_t cbft_ecdsa_p256_sign_launch(const EcdsaSignBatch& b, const uint32_t* d_tbl, uint32_t* d_scratch,
                                       uint8_t* d_sig, hipStream_t stream) {
  if (b.n == 0) return hipSuccess;
  const dim3 grid((unsigned)((b.n + P2S_BLOCK - 1) / P2S_BLOCK)), block(P2S_BLOCK);
  uint32_t* sig = reinterpret_cast<uint32_t*>(d_sig);
  hipLaunchKernelGGL(ecdsa_p256_sign_nonce_kernel, grid, block, 0, stream, b, d_scratch);
  hipLaunchKernelGGL(ecdsa_p256_sign_point_kernel, grid, block, 0, stream, b, d_tbl, d_scratch, sig);
  hipLaunchKernelGGL(ecdsa_p256_sign_redo_kernel, grid, block, 0, stream, b, d_tbl, d_scratch, sig);
  return hipGetLastError();
}
