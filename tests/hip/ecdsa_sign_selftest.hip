// Test-only device harness (not part of the product library): the ECDSA signing lane routines of
// csrc/ecdsa_sign.h for chosen inputs, one function per launch and one lane per input, so
// tests/test_ecdsa_sign_gpu.py can check on gfx950 what no message reaches through the C ABI:
// the nonce's retry path (a test order that refuses half of all candidates), signing with a chosen
// nonce, the comb on any 256-bit scalar and the two constant-time inversions, against
// tests/ecdsa_sign_ref.py and Python integers; and the product's batch launches (ecdsa_sign.hip,
// compiled in here) on a scratch of the harness's own, which is read back afterwards: the nonces
// must be gone from it.
//
// Operands are 8 little-endian words each; every lane writes ESS_OUT words:
//   [0..8) first result, [8..16) second result, [16] flag, [17..24) zero.
#include <hip/hip_runtime.h>

#include "ecdsa_sign.h"
#include "ecdsa_sign.hip"  // the product kernels and launches

#define ESS_OUT 24

__device__ __forceinline__ void ess_load(uint32_t* r, const uint32_t* p, int i) {
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = p[8 * i + j];
}
__device__ __forceinline__ void ess_put(uint32_t* out, int i, const uint32_t* a, const uint32_t* b, uint32_t flag) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    out[ESS_OUT * i + j] = a[j];
    out[ESS_OUT * i + 8 + j] = b[j];
    out[ESS_OUT * i + 16 + j] = j == 0 ? flag : 0u;
  }
}

__global__ void __launch_bounds__(128) ess_table_kernel(uint32_t* tbl) {
  if (blockIdx.x != 0 || threadIdx.x >= ECDSAS_TABLE_LANES) return;
  ecdsas_table_lane(tbl, (int)threadIdx.x);
}
// a = x, b = the digest as an integer, c = the order: k, zeros, the number of candidates refused
__global__ void __launch_bounds__(64) ess_nonce_kernel(const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                                       uint32_t* out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t x[8], z[8], q[8], h1[8], k[8], zero[8];
  ess_load(x, a, i);
  ess_load(z, b, i);
  ess_load(q, c, i);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    h1[j] = z[7 - j];
    zero[j] = 0u;
  }
  const uint32_t refused = ecdsas_nonce(k, x, h1, q);
  ess_put(out, i, k, zero, refused);
}
// a = x, b = e (< n), c = k: r, s, 1; or zeros and 0 for "next candidate"
__global__ void __launch_bounds__(64) ess_sign_with_k_kernel(const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                                             uint32_t* out, int n, const uint32_t* __restrict__ tbl) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t x[8], k[8];
  K1Sc e, r, s;
  ess_load(x, a, i);
  ess_load(e.v, b, i);
  ess_load(k, c, i);
  const uint32_t ok = ecdsas_sign_with_k(r, s, x, e, k, tbl);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    r.v[j] &= ok;
    s.v[j] &= ok;
  }
  ess_put(out, i, r.v, s.v, ok & 1u);
}
// a = k (any 256-bit value): affine x, y of k G, flag 1 for infinity (x = y = 0 then)
__global__ void __launch_bounds__(64) ess_comb_kernel(const uint32_t* a, uint32_t* out, int n,
                                                      const uint32_t* __restrict__ tbl) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t k[8];
  ess_load(k, a, i);
  K1Proj P;
  ecdsas_comb(P, k, tbl);
  K1Fe zi, x, y;
  fe_inv_ct(zi, P.z);
  fe_mul(x, P.x, zi);
  fe_mul(y, P.y, zi);
  ess_put(out, i, x.v, y.v, fe_is_zero(P.z) ? 1u : 0u);
}
// which = 0: a^-1 mod p; 1: a^-1 mod n
__global__ void __launch_bounds__(64) ess_inv_kernel(const uint32_t* a, uint32_t* out, int n, int which) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t zero[8];
#pragma unroll
  for (int j = 0; j < 8; j++) zero[j] = 0u;
  if (which == 0) {  // (public test switch)
    K1Fe x, r;
    ess_load(x.v, a, i);
    fe_inv_ct(r, x);
    ess_put(out, i, r.v, zero, 0u);
  } else {
    K1Sc x, r;
    ess_load(x.v, a, i);
    sc_inv_ct(r, x);
    ess_put(out, i, r.v, zero, 0u);
  }
}

// op: 0 nonce, 1 sign with k, 2 comb, 3 inverse mod p, 4 inverse mod n.  h_a, h_b, h_c: n x 8 words
// (h_b, h_c unused by ops 2..4); h_out: n x ESS_OUT words, uploaded as the caller filled it, so a
// lane that wrote nothing shows.  0 or a HIP error.
extern "C" int ecdsa_sign_selftest(int op, const uint32_t* h_a, const uint32_t* h_b, const uint32_t* h_c,
                                   uint32_t* h_out, int n) {
  if (n <= 0 || op < 0 || op > 4) return 0;
  const size_t bytes = (size_t)n * 8 * sizeof(uint32_t), obytes = (size_t)n * ESS_OUT * sizeof(uint32_t);
  uint32_t *d_a = nullptr, *d_b = nullptr, *d_c = nullptr, *d_out = nullptr, *d_tbl = nullptr;
  hipError_t e = hipMalloc(&d_a, bytes);
  if (e == hipSuccess) e = hipMalloc(&d_b, bytes);
  if (e == hipSuccess) e = hipMalloc(&d_c, bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, obytes);
  if (e == hipSuccess) e = hipMalloc(&d_tbl, (size_t)ECDSAS_TABLE_WORDS * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpy(d_a, h_a, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && op < 2) e = hipMemcpy(d_b, h_b, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && op < 2) e = hipMemcpy(d_c, h_c, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_out, h_out, obytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const dim3 grid((n + 63) / 64), block(64);
    if (op == 1 || op == 2) hipLaunchKernelGGL(ess_table_kernel, dim3(1), dim3(128), 0, 0, d_tbl);
    if (op == 0) hipLaunchKernelGGL(ess_nonce_kernel, grid, block, 0, 0, d_a, d_b, d_c, d_out, n);
    if (op == 1) hipLaunchKernelGGL(ess_sign_with_k_kernel, grid, block, 0, 0, d_a, d_b, d_c, d_out, n, d_tbl);
    if (op == 2) hipLaunchKernelGGL(ess_comb_kernel, grid, block, 0, 0, d_a, d_out, n, d_tbl);
    if (op >= 3) hipLaunchKernelGGL(ess_inv_kernel, grid, block, 0, 0, d_a, d_out, n, op - 3);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h_out, d_out, obytes, hipMemcpyDeviceToHost);
  for (uint32_t* p : {d_a, d_b, d_c, d_out, d_tbl}) (void)hipFree(p);
  return (int)e;
}

// The product's table, signer and batch launches for n messages of `len` bytes under priv[idx[i]]
// (idx null: signer 0): signatures to h_sig (n x 64 B) and the whole batch scratch, as the last
// kernel left it, to h_scratch (cbft_ecdsa_sign_scratch_words(n) words: k | h1 | state).
extern "C" int ecdsa_sign_selftest_batch(const uint8_t* h_priv, uint32_t nkeys, const uint32_t* h_idx, const uint8_t* h_msg,
                                         uint32_t len, int n, uint8_t* h_sig, uint32_t* h_scratch) {
  if (n <= 0 || nkeys == 0) return 0;
  const size_t sw = cbft_ecdsa_sign_scratch_words((size_t)n);
  uint8_t *d_priv = nullptr, *d_msg = nullptr, *d_sig = nullptr;
  uint32_t *d_idx = nullptr, *d_tbl = nullptr, *d_rec = nullptr, *d_scr = nullptr;
  hipError_t e = hipMalloc(&d_priv, (size_t)nkeys * 32);
  if (e == hipSuccess) e = hipMalloc(&d_msg, (size_t)n * len + 16);
  if (e == hipSuccess) e = hipMalloc(&d_sig, (size_t)n * 64);
  if (e == hipSuccess) e = hipMalloc(&d_idx, (size_t)n * 4);
  if (e == hipSuccess) e = hipMalloc(&d_tbl, (size_t)ECDSAS_TABLE_WORDS * 4);
  if (e == hipSuccess) e = hipMalloc(&d_rec, (size_t)nkeys * ECDSAS_WORDS * 4);
  if (e == hipSuccess) e = hipMalloc(&d_scr, sw * 4);
  if (e == hipSuccess) e = hipMemcpy(d_priv, h_priv, (size_t)nkeys * 32, hipMemcpyHostToDevice);
  if (e == hipSuccess && len) e = hipMemcpy(d_msg, h_msg, (size_t)n * len, hipMemcpyHostToDevice);
  if (e == hipSuccess && h_idx) e = hipMemcpy(d_idx, h_idx, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_scr, 0xA5, sw * 4);
  if (e == hipSuccess) e = cbft_ecdsa_sign_build_table(d_tbl, 0);
  if (e == hipSuccess) e = cbft_ecdsa_sign_launch_keys(d_priv, nkeys, d_tbl, d_rec, 0);
  if (e == hipSuccess) {
    const EcdsaSignBatch b{(size_t)n, d_rec, nkeys, h_idx ? d_idx : nullptr, d_msg, nullptr, nullptr, len};
    e = cbft_ecdsa_sign_launch(b, d_tbl, d_scr, d_sig, 0);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h_sig, d_sig, (size_t)n * 64, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(h_scratch, d_scr, sw * 4, hipMemcpyDeviceToHost);
  for (void* p : {(void*)d_priv, (void*)d_msg, (void*)d_sig, (void*)d_idx, (void*)d_tbl, (void*)d_rec, (void*)d_scr})
    (void)hipFree(p);
  return (int)e;
}
