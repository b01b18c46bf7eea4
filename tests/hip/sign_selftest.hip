// Test-only device harness (not part of the product library): the signing comb encode([r]B) and
// sc_muladd of csrc/ed25519_sign.h / sc25519.h for chosen inputs, one lane per input, so
// tests/test_ed25519_sign_gpu.py can check on gfx950 the arithmetic edges a SHA-512 output never
// reaches (r = 0, digits all -8 or all +7, r and k at L - 1, ...) against oracle/ed25519_ref.py
// and Python integers.
#include <hip/hip_runtime.h>

#define CBFT_SIGN_DEVICE_HELPERS
#include "ed25519_sign.h"

__global__ void __launch_bounds__(64) selftest_table_kernel(uint32_t* tbl) {
  if (blockIdx.x != 0 || threadIdx.x >= CBFT_SIGN_NPOS) return;
  sign_table_build_lane(tbl, (int)threadIdx.x);
}

// biased = 0: in is the scalar r (r + 0x88..8 < 2^256).  biased = 1: in is r + 0x88..8 itself,
// i.e. its 64 nibbles minus 8 are the signed digits (all-zero input = every digit -8).
__global__ void __launch_bounds__(64) selftest_mul_kernel(const uint32_t* in, uint32_t* out, int n, int biased,
                                                          const uint32_t* __restrict__ tbl) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t k[8], kp[9], o[8];
#pragma unroll
  for (int j = 0; j < 8; j++) k[j] = in[8 * i + j];
  sc_recode_prepare<CBFT_SIGN_W, CBFT_SIGN_NPOS>(kp, k);
  if (biased) {  // (public test switch)
    kp[0] = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) kp[j + 1] = k[j];
  }
  ge_p3 P;
  sign_comb_mul(P, kp, tbl);
  ge_tobytes(o, P.X, P.Y, P.Z);
#pragma unroll
  for (int j = 0; j < 8; j++) out[8 * i + j] = o[j];
}

__global__ void __launch_bounds__(64) selftest_muladd_kernel(const uint32_t* r, const uint32_t* k, const uint32_t* a,
                                                             uint32_t* out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t rr[8], kk[8], aa[8], s[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    rr[j] = r[8 * i + j];
    kk[j] = k[8 * i + j];
    aa[j] = a[8 * i + j];
  }
  sc_muladd(s, rr, kk, aa);
#pragma unroll
  for (int j = 0; j < 8; j++) out[8 * i + j] = s[j];
}

// n scalars of 8 little-endian words -> n encoded points (8 words each).  0 or a HIP error.
extern "C" int sign_selftest_mul(const uint32_t* h_in, uint32_t* h_out, int n, int biased) {
  if (n <= 0) return 0;
  const size_t bytes = (size_t)n * 8 * sizeof(uint32_t);
  uint32_t *d_in = nullptr, *d_out = nullptr, *d_tbl = nullptr;
  hipError_t e = hipMalloc(&d_in, bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, bytes);
  if (e == hipSuccess) e = hipMalloc(&d_tbl, (size_t)CBFT_SIGN_TABLE_WORDS * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpy(d_in, h_in, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(selftest_table_kernel, dim3(1), dim3(64), 0, 0, d_tbl);
    hipLaunchKernelGGL(selftest_mul_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, d_in, d_out, n, biased, d_tbl);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h_out, d_out, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  (void)hipFree(d_tbl);
  return (int)e;
}

// n triples (8 words each) -> (r + k a) mod L
extern "C" int sign_selftest_muladd(const uint32_t* h_r, const uint32_t* h_k, const uint32_t* h_a, uint32_t* h_out,
                                    int n) {
  if (n <= 0) return 0;
  const size_t bytes = (size_t)n * 8 * sizeof(uint32_t);
  uint32_t* d[4] = {nullptr, nullptr, nullptr, nullptr};
  const uint32_t* h[3] = {h_r, h_k, h_a};
  hipError_t e = hipSuccess;
  for (int j = 0; j < 4 && e == hipSuccess; j++) e = hipMalloc(&d[j], bytes);
  for (int j = 0; j < 3 && e == hipSuccess; j++) e = hipMemcpy(d[j], h[j], bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(selftest_muladd_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, d[0], d[1], d[2], d[3], n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h_out, d[3], bytes, hipMemcpyDeviceToHost);
  for (int j = 0; j < 4; j++) (void)hipFree(d[j]);
  return (int)e;
}
