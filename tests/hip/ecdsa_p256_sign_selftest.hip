// Test-only device harness (not part of the product library): the ECDSA P-256 signing lane routines
// of csrc/ecdsa_p256_sign.h for chosen inputs, one function per launch and one lane per input, so
// tests/test_ecdsa_p256_sign_gpu.py can check on gfx950 what no message reaches through the C ABI:
// the complete addition on infinity, equal and opposite points, b a, the two constant-time
// inversions, the comb on any 256-bit scalar, r = x mod n at and above n, signing with a chosen
// nonce, the s = 0 retry of the lane routine and the nonce's retry path (a test order that refuses
// half of all candidates), against tests/p256_sign_ref.py and Python integers; and the product's
// batch launches (ecdsa_p256_sign.hip, compiled in here) on a scratch of the harness's own, which is
// read back afterwards: the nonces must be gone from it.
//
// Operands are 8 little-endian words each; every lane writes P2T_OUT words:
//   [0..8) first result, [8..16) second, [16..24) third, [24] flag, [25..32) zero.
#include <hip/hip_runtime.h>

#include "ecdsa_p256_sign.h"
#include "ecdsa_p256_sign.hip"  // the product kernels and launches

#define P2T_OUT 32

__device__ __forceinline__ void p2t_load(uint32_t* r, const uint32_t* p, int i) {
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = p[8 * i + j];
}
__device__ __forceinline__ void p2t_put(uint32_t* out, int i, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                        uint32_t flag) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    out[P2T_OUT * i + j] = a[j];
    out[P2T_OUT * i + 8 + j] = b[j];
    out[P2T_OUT * i + 16 + j] = c[j];
    out[P2T_OUT * i + 24 + j] = j == 0 ? flag : 0u;
  }
}
__device__ __forceinline__ void p2t_zero(uint32_t* z) {
#pragma unroll
  for (int j = 0; j < 8; j++) z[j] = 0u;
}

// a = x, b = the digest as an integer, c = the order: k, zeros, zeros, the number of candidates refused
__global__ void __launch_bounds__(64) p2t_nonce_kernel(const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                                       uint32_t* out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t x[8], z[8], q[8], h1[8], k[8], zero[8];
  p2t_load(x, a, i);
  p2t_load(z, b, i);
  p2t_load(q, c, i);
  p2t_zero(zero);
#pragma unroll
  for (int j = 0; j < 8; j++) h1[j] = z[7 - j];
  const uint32_t refused = ecdsas_nonce(k, x, h1, q);
  p2t_put(out, i, k, zero, zero, refused);
}
// a = x, b = e (< n), c = k: r, s as computed, zeros, 1; flag 0 for "next candidate"
__global__ void __launch_bounds__(64) p2t_sign_with_k_kernel(const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                                             uint32_t* out, int n, const uint32_t* __restrict__ tbl) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t x[8], k[8], zero[8];
  P2Sc e, r, s;
  p2t_load(x, a, i);
  p2t_load(e.v, b, i);
  p2t_load(k, c, i);
  p2t_zero(zero);
  const uint32_t ok = p2s_sign_with_k(r, s, x, e, k, tbl);
  p2t_put(out, i, r.v, s.v, zero, ok & 1u);
}
// a = k (any 256-bit value): affine x, y of k G, zeros, flag 1 for infinity (x = y = 0 then)
__global__ void __launch_bounds__(64) p2t_comb_kernel(const uint32_t* a, uint32_t* out, int n,
                                                      const uint32_t* __restrict__ tbl) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t k[8], zero[8];
  p2t_load(k, a, i);
  p2t_zero(zero);
  P2Proj P;
  p2s_comb(P, k, tbl);
  P2Fe zi, x, y;
  p2s_fe_inv_ct(zi, P.z);
  p2_fe_mul(x, P.x, zi);
  p2_fe_mul(y, P.y, zi);
  p2t_put(out, i, x.v, y.v, zero, p2_fe_is_zero(P.z) ? 1u : 0u);
}
// which = 0: a^-1 mod p; 1: a^-1 mod n; 2: b a mod p; 3: a mod n for a field element a
__global__ void __launch_bounds__(64) p2t_unary_kernel(const uint32_t* a, uint32_t* out, int n, int which) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t zero[8], res[8];
  p2t_zero(zero);
  if (which == 0) {  // (public test switch)
    P2Fe x, r;
    p2t_load(x.v, a, i);
    p2s_fe_inv_ct(r, x);
    p2t_load(res, r.v, 0);
  } else if (which == 1) {
    P2Sc x, r;
    p2t_load(x.v, a, i);
    p2s_sc_inv_ct(r, x);
    p2t_load(res, r.v, 0);
  } else if (which == 2) {
    P2Fe x, r;
    p2t_load(x.v, a, i);
    p2s_fe_mulb(r, x);
    p2t_load(res, r.v, 0);
  } else {
    P2Fe x;
    P2Sc r;
    p2t_load(x.v, a, i);
    p2s_x_mod_n(r, x);
    p2t_load(res, r.v, 0);
  }
  p2t_put(out, i, res, zero, zero, 0u);
}
// (a : b : c) + (d, e) by the complete addition: X3, Y3, Z3 as they stand
__global__ void __launch_bounds__(64) p2t_madd_kernel(const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                                      const uint32_t* d, const uint32_t* e, uint32_t* out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  P2Proj p, r;
  P2Fe qx, qy;
  p2t_load(p.x.v, a, i);
  p2t_load(p.y.v, b, i);
  p2t_load(p.z.v, c, i);
  p2t_load(qx.v, d, i);
  p2t_load(qy.v, e, i);
  p2s_madd(r, p, qx, qy);
  p2t_put(out, i, r.x.v, r.y.v, r.z.v, 0u);
}
// a = x, b = the digest as an integer (it seeds the generator), c = e (enters s): the lane routine's r, s
__global__ void __launch_bounds__(64) p2t_sign_lane_e_kernel(const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                                             uint32_t* out, int n, const uint32_t* __restrict__ tbl) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t x[8], z[8], h1[8], sig[16], r[8], s[8], zero[8];
  P2Sc e;
  p2t_load(x, a, i);
  p2t_load(z, b, i);
  p2t_load(e.v, c, i);
  p2t_zero(zero);
#pragma unroll
  for (int j = 0; j < 8; j++) h1[j] = z[7 - j];
  p2s_sign_lane_e(sig, x, h1, e, tbl);
#pragma unroll
  for (int j = 0; j < 8; j++) {  // back to limbs
    r[j] = __builtin_bswap32(sig[7 - j]);
    s[j] = __builtin_bswap32(sig[15 - j]);
  }
  p2t_put(out, i, r, s, zero, 1u);
}

// op: 0 nonce (a, b, c), 1 sign with k (a, b, c), 2 comb (a), 3 inverse mod p, 4 inverse mod n, 5 b a, 6 a mod n (a),
// 7 complete addition (a, b, c, d, e), 8 the lane routine with e given apart (a, b, c).  Every h_* is n x 8 words
// (unused ones may be null); h_out: n x P2T_OUT words, uploaded as the caller filled it, so a lane that wrote
// nothing shows.  0 or a HIP error.
extern "C" int ecdsa_p256_sign_selftest(int op, const uint32_t* h_a, const uint32_t* h_b, const uint32_t* h_c,
                                        const uint32_t* h_d, const uint32_t* h_e, uint32_t* h_out, int n) {
  if (n <= 0 || op < 0 || op > 8 || !h_a || !h_out) return 0;
  const int nin = (op == 7) ? 5 : (op == 0 || op == 1 || op == 8) ? 3 : 1;
  const uint32_t* h_in[5] = {h_a, h_b, h_c, h_d, h_e};
  for (int k = 0; k < nin; k++)
    if (!h_in[k]) return -1;
  const size_t bytes = (size_t)n * 8 * sizeof(uint32_t), obytes = (size_t)n * P2T_OUT * sizeof(uint32_t);
  uint32_t* d_in[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  uint32_t *d_out = nullptr, *d_tbl = nullptr;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 5 && e == hipSuccess; k++) e = hipMalloc(&d_in[k], bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, obytes);
  if (e == hipSuccess) e = hipMalloc(&d_tbl, (size_t)ECDSAS_TABLE_WORDS * sizeof(uint32_t));
  for (int k = 0; k < nin && e == hipSuccess; k++) e = hipMemcpy(d_in[k], h_in[k], bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_out, h_out, obytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const dim3 grid((n + 63) / 64), block(64);
    if (op == 1 || op == 2 || op == 8) e = cbft_ecdsa_p256_sign_build_table(d_tbl, 0);
    if (op == 0) hipLaunchKernelGGL(p2t_nonce_kernel, grid, block, 0, 0, d_in[0], d_in[1], d_in[2], d_out, n);
    if (op == 1) hipLaunchKernelGGL(p2t_sign_with_k_kernel, grid, block, 0, 0, d_in[0], d_in[1], d_in[2], d_out, n, d_tbl);
    if (op == 2) hipLaunchKernelGGL(p2t_comb_kernel, grid, block, 0, 0, d_in[0], d_out, n, d_tbl);
    if (op >= 3 && op <= 6) hipLaunchKernelGGL(p2t_unary_kernel, grid, block, 0, 0, d_in[0], d_out, n, op - 3);
    if (op == 7)
      hipLaunchKernelGGL(p2t_madd_kernel, grid, block, 0, 0, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], d_out, n);
    if (op == 8) hipLaunchKernelGGL(p2t_sign_lane_e_kernel, grid, block, 0, 0, d_in[0], d_in[1], d_in[2], d_out, n, d_tbl);
    if (e == hipSuccess) e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h_out, d_out, obytes, hipMemcpyDeviceToHost);
  for (uint32_t* p : {d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], d_out, d_tbl}) (void)hipFree(p);
  return (int)e;
}

// The product's table, signer and batch launches for n messages of `len` bytes under priv[idx[i]]
// (idx null: signer 0): signatures to h_sig (n x 64 B) and the whole batch scratch, as the last
// kernel left it, to h_scratch (cbft_ecdsa_sign_scratch_words(n) words: k | h1 | state).
extern "C" int ecdsa_p256_sign_selftest_batch(const uint8_t* h_priv, uint32_t nkeys, const uint32_t* h_idx,
                                              const uint8_t* h_msg, uint32_t len, int n, uint8_t* h_sig,
                                              uint32_t* h_scratch) {
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
  if (e == hipSuccess) e = cbft_ecdsa_p256_sign_build_table(d_tbl, 0);
  if (e == hipSuccess) e = cbft_ecdsa_p256_sign_launch_keys(d_priv, nkeys, d_tbl, d_rec, 0);
  if (e == hipSuccess) {
    const EcdsaSignBatch b{(size_t)n, d_rec, nkeys, h_idx ? d_idx : nullptr, d_msg, nullptr, nullptr, len};
    e = cbft_ecdsa_p256_sign_launch(b, d_tbl, d_scr, d_sig, 0);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h_sig, d_sig, (size_t)n * 64, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(h_scratch, d_scr, sw * 4, hipMemcpyDeviceToHost);
  for (void* p : {(void*)d_priv, (void*)d_msg, (void*)d_sig, (void*)d_idx, (void*)d_tbl, (void*)d_rec, (void*)d_scr})
    (void)hipFree(p);
  return (int)e;
}
