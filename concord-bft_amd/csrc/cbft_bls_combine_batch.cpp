// libcbft_hipcrypto, batched BLS share combination half of the C ABI (include/cbft_hipcrypto.h).
//
// The batch form of IThresholdAccumulator::getFullSignedData: a collector with a window of sequence
// numbers open, and a view change or checkpoint that rebuilds many certificates, hold many
// certificates of few shares each (n = 4 .. 31 replicas, k = 3 .. 21).  One call combines m of them,
// one share per lane (bls_combine_batch.hip); cbft_bls_combine stays the call for one large
// certificate.  With the verdict bytes of cbft_bls_verify_fixed_device as `use`, a window's shares
// go verify -> combine -> verify on the device without a host round trip.
//
// Multi-GPU contexts: the host form cuts the certificates into contiguous slices, one per device;
// the _device entry needs a single-GPU context.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "bls_combine_batch.h"
#include "bls_kernels.h"
#include "cbft_internal.h"

void cbft_bls_combine_batch_release(cbft_ctx* c) {
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();  // device-path batches run on caller streams
  for (DevBuf* b : {&c->blsc.in, &c->blsc.out}) b->release();
  c->blsc.scratch.release();
}

// the argument checks of the host form that need no device: CBFT_EINVAL / CBFT_E2BIG before anything is launched
static int blsc_check(const uint64_t* off, size_t m) {
  for (size_t c = 0; c < m; c++)
    if (off[c + 1] < off[c] || off[c + 1] - off[c] > BLS_COMBINE_MAX_K) return CBFT_EINVAL;
  if (m && off[m] - off[0] > BLS_COMBINE_BATCH_MAX) return CBFT_E2BIG;
  return CBFT_OK;
}

// the inverses of 1 .. 2048 mod r, once per context (cbft_bls_combine builds the same table): ready for
// every stream when this returns
static int blsc_inv_locked(cbft_ctx* c) {
  if (c->bls_inv.p) return CBFT_OK;
  CBFT_HIP(c->bls_inv.reserve((size_t)BLS_INV_TABLE * 9 * 4));
  CBFT_HIP(cbft_bls_launch_inv_table(c->bls_inv.as<uint32_t>(), c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  return CBFT_OK;
}

static int blsc_launch_locked(cbft_ctx* c, BlsCombineBatch b, hipStream_t s) {
  if (!b.multisig) {
    const int rc = blsc_inv_locked(c);
    if (rc) return rc;
    b.inv = c->bls_inv.as<uint32_t>();
  }
  CBFT_HIP(c->blsc.scratch.acquire(cbft_bls_combine_batch_scratch_bytes(b.n), s));
  CBFT_HIP(cbft_bls_combine_batch_launch(b, c->blsc.scratch.buf.p, s));
  CBFT_HIP(c->blsc.scratch.commit(s));
  return CBFT_OK;
}

// one device, host arrays: certificates off[0 .. m] (absolute share indices into shares37 / use)
static int blsc_host_one(cbft_ctx* c, const uint8_t* shares37, const uint64_t* off, size_t m, const uint8_t* use,
                         int multisig, uint8_t* out33, uint8_t* status) {
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  std::vector<uint32_t> off32;
  for (size_t c0 = 0; c0 < m;) {
    // whole certificates while the launch sequence's share cap holds (one certificate always fits)
    size_t c1 = c0 + 1;
    while (c1 < m && c1 - c0 < BLS_COMBINE_LAUNCH_MAX && off[c1 + 1] - off[c0] <= BLS_COMBINE_LAUNCH_MAX) c1++;
    const size_t mc = c1 - c0, n = off[c1] - off[c0];
    off32.resize(mc + 1);
    for (size_t i = 0; i <= mc; i++) off32[i] = (uint32_t)(off[c0 + i] - off[c0]);
    // device image: offsets (mc + 1 words) | shares 37 n | use n
    const size_t at_sh = (mc + 1) * 4, at_use = at_sh + 37 * n;
    CBFT_HIP(c->blsc.in.reserve(at_use + n));
    CBFT_HIP(c->blsc.out.reserve(34 * mc));
    uint8_t* d = c->blsc.in.as<uint8_t>();
    CBFT_HIP(hipMemcpyAsync(d, off32.data(), at_sh, hipMemcpyHostToDevice, c->stream));
    if (n) CBFT_HIP(hipMemcpyAsync(d + at_sh, shares37 + 37 * off[c0], 37 * n, hipMemcpyHostToDevice, c->stream));
    if (n && use) CBFT_HIP(hipMemcpyAsync(d + at_use, use + off[c0], n, hipMemcpyHostToDevice, c->stream));
    BlsCombineBatch b{};
    b.n = (uint32_t)n;
    b.m = (uint32_t)mc;
    b.shares = d + at_sh;
    b.use = use ? d + at_use : nullptr;
    b.off = reinterpret_cast<const uint32_t*>(d);
    b.multisig = multisig;
    b.out33 = c->blsc.out.as<uint8_t>();
    b.status = b.out33 + 33 * mc;
    const int rc = blsc_launch_locked(c, b, c->stream);
    if (rc) return rc;
    CBFT_HIP(hipMemcpyAsync(out33 + 33 * c0, b.out33, 33 * mc, hipMemcpyDeviceToHost, c->stream));
    CBFT_HIP(hipMemcpyAsync(status + c0, b.status, mc, hipMemcpyDeviceToHost, c->stream));
    CBFT_HIP(hipStreamSynchronize(c->stream));  // off32 and the device image are reused by the next part
    c0 = c1;
  }
  return CBFT_OK;
}

extern "C" {

int cbft_bls_combine_batch(cbft_ctx* c, const uint8_t* shares37, const uint64_t* cert_off, size_t m, const uint8_t* use,
                           int multisig, uint8_t* out33, uint8_t* status) {
  if (!c || (m && (!shares37 || !cert_off || !out33 || !status))) return CBFT_EINVAL;
  if (!m) return CBFT_OK;
  const int rc0 = blsc_check(cert_off, m);
  if (rc0) return rc0;
  if (c->kids.empty()) return blsc_host_one(c, shares37, cert_off, m, use, multisig, out33, status);
  // multi-GPU: every check is done; one contiguous slice of certificates per device
  const size_t G = c->kids.size(), per = (m + G - 1) / G;
  return for_each_kid(c, [&](size_t g) {
    const size_t lo = std::min(m, g * per), hi = std::min(m, lo + per);
    if (hi == lo) return (int)CBFT_OK;
    return blsc_host_one(c->kids[g], shares37, cert_off + lo, hi - lo, use, multisig, out33 + 33 * lo, status + lo);
  });
}

int cbft_bls_combine_fixed_device(cbft_ctx* c, const uint8_t* d_shares37, uint32_t k, size_t m, const uint8_t* d_use,
                                  int multisig, uint8_t* d_out33, uint8_t* d_status, void* stream) {
  if (c && !c->kids.empty()) return CBFT_EINVAL;  // device pointers belong to one GPU: use its own context
  if (!c || (m && (!d_out33 || !d_status)) || (m && k && !d_shares37) || k > BLS_COMBINE_MAX_K) return CBFT_EINVAL;
  if (m > BLS_COMBINE_BATCH_MAX || (uint64_t)m * k > BLS_COMBINE_BATCH_MAX) return CBFT_E2BIG;
  if (!m) return CBFT_OK;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  const size_t per = k ? std::max<size_t>(1, BLS_COMBINE_LAUNCH_MAX / k) : BLS_COMBINE_LAUNCH_MAX;
  for (size_t c0 = 0; c0 < m; c0 += per) {
    const size_t mc = std::min(per, m - c0);
    BlsCombineBatch b{};
    b.n = (uint32_t)(mc * k);
    b.m = (uint32_t)mc;
    b.shares = d_shares37 + 37 * c0 * k;
    b.use = d_use ? d_use + c0 * k : nullptr;
    b.k = k;
    b.multisig = multisig;
    b.out33 = d_out33 + 33 * c0;
    b.status = d_status + c0;
    const int rc = blsc_launch_locked(c, b, s);
    if (rc) return rc;
  }
  return CBFT_OK;
}

}  // extern "C"
