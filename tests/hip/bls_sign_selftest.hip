// Test-only device harness of the batched BLS signing lane code (csrc/bls_sign_batch.h), for what
// the product entry points cannot reach (tests/test_bls_sign_gpu.py, tools/bls_sign_bench.py):
//   - try-and-increment from a GIVEN x (a hash never produces 0, 1, p - 1, ..);
//   - the product kernels beside their rejected variants (plain hash loop; window 4 with the table
//     in LDS or in global scratch), each timed
//     with events around it and with the hash kernel's rounds per block.
// Not part of the product library.
#include <hip/hip_runtime.h>

#include <vector>

#include "bls_sign_batch.h"

#define ST_HIP(x)                    \
  do {                               \
    hipError_t e_ = (x);             \
    if (e_ != hipSuccess) return -(int)e_ - 1000; \
  } while (0)

// x: n x 8 LE words (< p).  out: n x 17 words = final x (8, canonical), y (8, canonical), increments
__global__ void __launch_bounds__(64) st_map_from_x_kernel(const uint32_t* xw, uint32_t n, uint32_t* out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  for (int q = 0; q < 8; q++) w[q] = xw[8 * (size_t)i + q];
  fp x, y;
  f_from_words(x, w);
  uint32_t inc = 0;
  while (!bls_map_try(y, x)) inc++;
  f_to_words(w, x);
  for (int q = 0; q < 8; q++) out[17 * (size_t)i + q] = w[q];
  f_to_words(w, y);
  for (int q = 0; q < 8; q++) out[17 * (size_t)i + 8 + q] = w[q];
  out[17 * (size_t)i + 16] = inc;
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

int bls_sign_selftest_map_from_x(const uint32_t* xw, uint32_t n, uint32_t* out17) {
  Dev<uint32_t> dx, dout;
  ST_HIP(dx.alloc(8 * (size_t)n));
  ST_HIP(dout.alloc(17 * (size_t)n));
  ST_HIP(hipMemcpy(dx.p, xw, 32 * (size_t)n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(st_map_from_x_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, dx.p, n, dout.p);
  ST_HIP(hipGetLastError());
  ST_HIP(hipDeviceSynchronize());
  ST_HIP(hipMemcpy(out17, dout.p, 68 * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

// n fixed-length messages under the record rec12 (bls_sign_shim_record), n <= BLS_SIGN_LAUNCH_MAX.
// steal picks the hash scheduling, (w, lds) the table geometry: (3, 1), (4, 1) or (4, 0); the product
// runs steal = 1, w = BLS_SIGN_W, lds = 1.
// out37: n x 37; ms[0] / ms[1]: the hash / multiplication kernel's time over `reps` timed runs after one
// untimed; rounds: ceil(n / 256) words, the hash kernel's rounds per block.
int bls_sign_selftest_variant(int steal, int w, int lds, const uint32_t* rec12, const uint8_t* msgs, uint32_t msg_len,
                              uint32_t n, int reps, uint8_t* out37, float* ms, uint32_t* rounds) {
  if (n == 0 || n > BLS_SIGN_LAUNCH_MAX || reps < 1) return -1;
  if (!((w == 3 && lds) || w == 4)) return -1;
  const uint32_t hb = (n + BLS_SIGN_HASH_CHUNK - 1) / BLS_SIGN_HASH_CHUNK;
  Dev<uint32_t> drec, dH, dtbl, drounds;
  Dev<uint8_t> dmsg, dout;
  ST_HIP(drec.alloc(BLS_SIGNER_WORDS));
  ST_HIP(dH.alloc(18 * (size_t)n));
  ST_HIP(dtbl.alloc(lds ? 1 : BLS_SIGN_TBL_WORDS(4) * (size_t)n));
  ST_HIP(drounds.alloc(hb));
  ST_HIP(dmsg.alloc((size_t)n * msg_len));
  ST_HIP(dout.alloc(37 * (size_t)n));
  ST_HIP(hipMemcpy(drec.p, rec12, BLS_SIGNER_WORDS * 4, hipMemcpyHostToDevice));
  ST_HIP(hipMemcpy(dmsg.p, msgs, (size_t)n * msg_len, hipMemcpyHostToDevice));
  hipEvent_t ev[3];
  for (auto& e : ev) ST_HIP(hipEventCreate(&e));
  ms[0] = ms[1] = 0.f;
  for (int r = 0; r <= reps; r++) {
    ST_HIP(hipEventRecord(ev[0], 0));
    if (steal)
      hipLaunchKernelGGL(bls_sign_hash_kernel<true>, dim3(hb), dim3(64), 0, 0, dmsg.p, (const uint64_t*)nullptr,
                         (const uint32_t*)nullptr, msg_len, n, dH.p, drounds.p);
    else
      hipLaunchKernelGGL(bls_sign_hash_kernel<false>, dim3(hb), dim3(64), 0, 0, dmsg.p, (const uint64_t*)nullptr,
                         (const uint32_t*)nullptr, msg_len, n, dH.p, drounds.p);
    ST_HIP(hipGetLastError());
    ST_HIP(hipEventRecord(ev[1], 0));
    if (w == 3)
      hipLaunchKernelGGL((bls_sign_mul_kernel<3, true>), dim3((n + 63) / 64), dim3(64), 0, 0, n, drec.p, 1u,
                         (const uint32_t*)nullptr, dH.p, dtbl.p, dout.p);
    else if (lds)
      hipLaunchKernelGGL((bls_sign_mul_kernel<4, true>), dim3((n + 63) / 64), dim3(64), 0, 0, n, drec.p, 1u,
                         (const uint32_t*)nullptr, dH.p, dtbl.p, dout.p);
    else
      hipLaunchKernelGGL((bls_sign_mul_kernel<4, false>), dim3((n + 63) / 64), dim3(64), 0, 0, n, drec.p, 1u,
                         (const uint32_t*)nullptr, dH.p, dtbl.p, dout.p);
    ST_HIP(hipGetLastError());
    ST_HIP(hipEventRecord(ev[2], 0));
    ST_HIP(hipEventSynchronize(ev[2]));
    if (r) {
      float a = 0.f, b = 0.f;
      ST_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
      ST_HIP(hipEventElapsedTime(&b, ev[1], ev[2]));
      ms[0] += a / reps;
      ms[1] += b / reps;
    }
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  ST_HIP(hipMemcpy(out37, dout.p, 37 * (size_t)n, hipMemcpyDeviceToHost));
  ST_HIP(hipMemcpy(rounds, drounds.p, 4 * (size_t)hb, hipMemcpyDeviceToHost));
  ST_HIP(hipMemset(drec.p, 0, BLS_SIGNER_WORDS * 4));
  return 0;
}

}  // extern "C"
