// Test-only device harness of the RSA signing CRT core (csrc/rsa_sign.h rs_crt_core and
// rs_build_record) on raw message representatives that no message reaches: EM = 0, 1, n - 1,
// multiples of p or q, equal or ordered CRT halves.  Not part of the product library;
// tests/test_rsa_sign_gpu.py loads it.
#include <hip/hip_runtime.h>

#define CBFT_RSA_SIGN_DEVICE_HELPERS
#include "rsa_sign.h"

namespace {

__global__ void __launch_bounds__(64) keys_kernel(const uint8_t* priv, const uint32_t* exps, uint32_t nkeys,
                                                  uint32_t* recs, uint8_t* mod) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeys) return;
  rs_build_record(recs + (size_t)k * RSAS_WORDS, priv + (size_t)k * RSAS_PRIV_BYTES, exps[k], mod + (size_t)k * 256);
}

// item i: s = CRT(em[i]) under record key_idx[i] (in range by the caller's contract); lanes past
// the end work on item 0 and store nothing
__global__ void __launch_bounds__(64, 2) crt_kernel(const uint32_t* recs, const uint32_t* key_idx, const uint8_t* em,
                                                    uint32_t n, uint32_t* scratch, uint8_t* out) {
  const uint32_t tid = threadIdx.x;
  const uint32_t item = blockIdx.x * RSAS_PSIG + (tid >> 1);
  const bool live = item < n;
  const uint32_t si = live ? item : 0;
  const uint32_t* rec = recs + (size_t)key_idx[si] * RSAS_WORDS;
  uint32_t emw[64], em74[2 * RS_NL];
#pragma unroll
  for (int k = 0; k < 64; k++) emw[k] = rs_load_be32(em + (size_t)si * 256 + 256 - 4 * (k + 1));
#pragma unroll
  for (int i = 0; i < 2 * RS_NL; i++) em74[i] = rs_limb28<64>(emw, i);
  uint32_t s[64];
  rs_crt_core(s, rec, tid & 1, em74, scratch + (size_t)blockIdx.x * (64 * RSAS_TBL * RSAS_NL) + tid);
  if (live && !(tid & 1)) {
    uint32_t* o = reinterpret_cast<uint32_t*>(out + (size_t)item * 256);
#pragma unroll
    for (int k = 0; k < 64; k++) o[63 - k] = __builtin_bswap32(s[k]);
  }
}

}  // namespace

#define ST_HIP(x)                      \
  do {                                 \
    if ((x) != hipSuccess) goto fail;  \
  } while (0)

// Host arrays in, host arrays out.  priv: nkeys x 640 B; em: n x 256 B big-endian (< 2^2048);
// out: n x 256 B; out_mod: nkeys x 256 B (p q); out_struct: nkeys structural-check words;
// out_scratch_or: the OR of every scratch word after the run (0: the tables were cleared).
extern "C" int rsa_sign_selftest_crt(const uint8_t* priv, const uint32_t* exps, uint32_t nkeys,
                                     const uint32_t* key_idx, const uint8_t* em, uint32_t n, uint8_t* out,
                                     uint8_t* out_mod, uint32_t* out_struct, uint32_t* out_scratch_or) {
  uint8_t *d_priv = nullptr, *d_mod = nullptr, *d_em = nullptr, *d_out = nullptr;
  uint32_t *d_exp = nullptr, *d_rec = nullptr, *d_idx = nullptr, *d_scr = nullptr;
  const unsigned blocks = (n + RSAS_PSIG - 1) / RSAS_PSIG;
  const size_t scr_words = (size_t)blocks * 64 * RSAS_TBL * RSAS_NL;
  int rc = -1;
  for (uint32_t i = 0; i < n; i++)
    if (key_idx[i] >= nkeys) return -2;
  if (!n || !nkeys) return -2;
  {
    ST_HIP(hipMalloc(&d_priv, (size_t)nkeys * RSAS_PRIV_BYTES));
    ST_HIP(hipMalloc(&d_mod, (size_t)nkeys * 256));
    ST_HIP(hipMalloc(&d_exp, (size_t)nkeys * 4));
    ST_HIP(hipMalloc(&d_rec, (size_t)nkeys * RSAS_WORDS * 4));
    ST_HIP(hipMalloc(&d_idx, (size_t)n * 4));
    ST_HIP(hipMalloc(&d_em, (size_t)n * 256));
    ST_HIP(hipMalloc(&d_out, (size_t)n * 256));
    ST_HIP(hipMalloc(&d_scr, scr_words * 4));
    ST_HIP(hipMemcpy(d_priv, priv, (size_t)nkeys * RSAS_PRIV_BYTES, hipMemcpyHostToDevice));
    ST_HIP(hipMemcpy(d_exp, exps, (size_t)nkeys * 4, hipMemcpyHostToDevice));
    ST_HIP(hipMemcpy(d_idx, key_idx, (size_t)n * 4, hipMemcpyHostToDevice));
    ST_HIP(hipMemcpy(d_em, em, (size_t)n * 256, hipMemcpyHostToDevice));
    ST_HIP(hipMemset(d_scr, 0xff, scr_words * 4));
    hipLaunchKernelGGL(keys_kernel, dim3((nkeys + 63) / 64), dim3(64), 0, 0, d_priv, d_exp, nkeys, d_rec, d_mod);
    ST_HIP(hipGetLastError());
    hipLaunchKernelGGL(crt_kernel, dim3(blocks), dim3(64), 0, 0, d_rec, d_idx, d_em, n, d_scr, d_out);
    ST_HIP(hipGetLastError());
    ST_HIP(hipDeviceSynchronize());
    ST_HIP(hipMemcpy(out, d_out, (size_t)n * 256, hipMemcpyDeviceToHost));
    if (out_mod) ST_HIP(hipMemcpy(out_mod, d_mod, (size_t)nkeys * 256, hipMemcpyDeviceToHost));
    if (out_struct)
      ST_HIP(hipMemcpy2D(out_struct, 4, d_rec + RSAS_STRUCT, RSAS_WORDS * 4, 4, nkeys, hipMemcpyDeviceToHost));
    if (out_scratch_or) {
      uint32_t* h = static_cast<uint32_t*>(malloc(scr_words * 4));
      if (!h) goto fail;
      if (hipMemcpy(h, d_scr, scr_words * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        free(h);
        goto fail;
      }
      uint32_t acc = 0;
      for (size_t i = 0; i < scr_words; i++) acc |= h[i];
      free(h);
      *out_scratch_or = acc;
    }
    rc = 0;
  }
fail:
  (void)hipMemset(d_priv, 0, d_priv ? (size_t)nkeys * RSAS_PRIV_BYTES : 0);
  if (d_rec) (void)hipMemset(d_rec, 0, (size_t)nkeys * RSAS_WORDS * 4);
  for (void* p : {(void*)d_priv, (void*)d_mod, (void*)d_em, (void*)d_out, (void*)d_exp, (void*)d_rec, (void*)d_idx,
                  (void*)d_scr})
    if (p) (void)hipFree(p);
  return rc;
}
