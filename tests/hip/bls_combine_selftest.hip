// Test-only device harness of the batched BLS combination (not the product library): the product's
// kernels (csrc/bls_combine_batch.hip, included as source) timed with events, whole and stage by stage
// (decode, Lagrange, lambda * sigma, sum + close), and beside the third stage the constant-time lane
// kernel of the batched signing (bls_sign_mul_kernel<BLS_SIGN_W, true>) on the same
// points.  tools/bls_combine_bench.py drives it.
#include "../../concord-bft_amd/csrc/bls_combine_batch.hip"

#include <vector>

#define ST_HIP(x)                    \
  do {                               \
    hipError_t _e = (x);             \
    if (_e != hipSuccess) {          \
      rc = (int)_e;                  \
      goto out;                      \
    }                                \
  } while (0)

// decoded shares (19 words each) -> the [word][n] hash-point layout the signing kernel reads
__global__ void __launch_bounds__(64) blsc_st_points_kernel(const uint32_t* sig, uint32_t n, uint32_t* H) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  for (int w = 0; w < 2 * BN_LIMBS; w++) H[(size_t)w * n + i] = sig[BLS_SIG_WORDS * (size_t)i + w];
}

// shares37: m x k shares (every one must decode to a finite point).  out33 / status: m.  ms_out[0]: the
// whole batch; ms_out[1..4]: decode, Lagrange, lambda * sigma, sum + close (events between the kernels of
// one launch sequence); ms_out[5]: the constant-time signing kernel over the same m k points under one
// record.  Best of reps each.  Returns 0 or a hipError_t.
extern "C" int blsc_selftest_run(const uint8_t* shares37, uint32_t k, uint32_t m, int multisig, uint8_t* out33,
                                 uint8_t* status, int reps, float* ms_out) {
  int rc = 0;
  const uint32_t n = m * k;
  uint8_t *d_sh = nullptr, *d_out = nullptr, *d_st = nullptr, *d_o37 = nullptr;
  uint32_t *d_inv = nullptr, *d_H = nullptr, *d_rec = nullptr;
  void* d_scr = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipStream_t s = nullptr;
  BlsCombineBatch b{};
  float best[6] = {1e30f, 1e30f, 1e30f, 1e30f, 1e30f, 1e30f};
  if (!n || n > BLS_COMBINE_LAUNCH_MAX || k > BLS_COMBINE_MAX_K || reps < 1) return -1;
  ST_HIP(hipStreamCreate(&s));
  for (hipEvent_t& e : ev) ST_HIP(hipEventCreate(&e));
  ST_HIP(hipMalloc(&d_sh, (size_t)n * 37));
  ST_HIP(hipMalloc(&d_out, (size_t)m * 33));
  ST_HIP(hipMalloc(&d_st, m));
  ST_HIP(hipMalloc(&d_inv, (size_t)BLS_INV_TABLE * 9 * 4));
  ST_HIP(hipMalloc(&d_scr, cbft_bls_combine_batch_scratch_bytes(n)));
  ST_HIP(hipMalloc(&d_H, (size_t)n * 2 * BN_LIMBS * 4));
  ST_HIP(hipMalloc(&d_rec, BLS_SIGNER_WORDS * 4));
  ST_HIP(hipMalloc(&d_o37, (size_t)n * 37));
  ST_HIP(hipMemcpyAsync(d_sh, shares37, (size_t)n * 37, hipMemcpyHostToDevice, s));
  ST_HIP(cbft_bls_launch_inv_table(d_inv, s));
  b.n = n;
  b.m = m;
  b.shares = d_sh;
  b.k = k;
  b.multisig = multisig;
  b.inv = d_inv;
  b.out33 = d_out;
  b.status = d_st;
  ST_HIP(cbft_bls_combine_batch_launch(b, d_scr, s));  // warm-up; its results are returned
  ST_HIP(hipMemcpyAsync(out33, d_out, (size_t)m * 33, hipMemcpyDeviceToHost, s));
  ST_HIP(hipMemcpyAsync(status, d_st, m, hipMemcpyDeviceToHost, s));
  ST_HIP(hipStreamSynchronize(s));
  {
    // one signer record (any scalar in [1, r)) for the constant-time kernel, built by the product's host code
    uint32_t rec[BLS_SIGNER_WORDS];
    const uint32_t sk[8] = {0x9e3779b9u, 0x7f4a7c15u, 0xbf58476du, 0x1ce4e5b9u, 0x94d049bbu, 0x133111ebu, 0x2545f491u, 0x0a5a5a5au};
    bls_signer_record(rec, sk, 1);
    ST_HIP(hipMemcpyAsync(d_rec, rec, sizeof rec, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(blsc_st_points_kernel, dim3((n + 63) / 64), dim3(64), 0, s, static_cast<uint32_t*>(d_scr), n, d_H);
    ST_HIP(hipGetLastError());
    ST_HIP(hipStreamSynchronize(s));
  }
  for (int r = 0; r < reps; r++) {
    ST_HIP(cbft_bls_combine_batch_launch(b, d_scr, s, ev));
    ST_HIP(hipEventSynchronize(ev[4]));
    float ms = 0;
    ST_HIP(hipEventElapsedTime(&ms, ev[0], ev[4]));
    if (ms < best[0]) best[0] = ms;
    for (int st = 0; st < 4; st++) {
      ST_HIP(hipEventElapsedTime(&ms, ev[st], ev[st + 1]));
      if (ms < best[1 + st]) best[1 + st] = ms;
    }
    ST_HIP(hipEventRecord(ev[0], s));
    hipLaunchKernelGGL((bls_sign_mul_kernel<BLS_SIGN_W, true>), dim3((n + 63) / 64), dim3(64), 0, s, n, d_rec, 1u,
                       (const uint32_t*)nullptr, d_H, (uint32_t*)nullptr, d_o37);
    ST_HIP(hipGetLastError());
    ST_HIP(hipEventRecord(ev[1], s));
    ST_HIP(hipEventSynchronize(ev[1]));
    ST_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    if (ms < best[5]) best[5] = ms;
  }
  for (int i = 0; i < 6; i++) ms_out[i] = best[i];
out:
  (void)hipDeviceSynchronize();
  for (void* p : {(void*)d_sh, (void*)d_out, (void*)d_st, (void*)d_inv, d_scr, (void*)d_H, (void*)d_rec, (void*)d_o37})
    if (p) (void)hipFree(p);
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  if (s) (void)hipStreamDestroy(s);
  return rc;
}
