// libcbft_hipcrypto, batched BLS key derivation and threshold key generation half of the C ABI
// (include/cbft_hipcrypto.h).
//
// The batch form of cbft_bls_public_key (vk = sk * g2, one key per lane: bls_keygen_batch.h) and
// BlsThresholdKeygen's Shamir dealing (sk_i = f(i), vk_i = sk_i * g2, PK = f(0) * g2) as one launch
// chain: coefficients -> Montgomery form, one share per lane by Horner, then the n + 1 keys.
//
// Multi-GPU contexts: all three entries run on the lowest device (cbft_dev0), like the signer tables;
// the _device entry needs a single-GPU context.
//
// Secrets: scalars and coefficients pass through pinned staging that is zeroed once the call's stream
// has drained; their device copies, the Montgomery coefficients and the dealt shares are cleared with
// hipMemsetAsync on the same stream before the call returns, on every exit path.  The device entry
// keeps nothing: its kernel reads the caller's scalars and writes the caller's keys, and the comb of g2
// it shares with the other entries is public and built once, so calls on different streams have no
// scratch to be ordered over.  The dealing's scratch is held by a ScratchGuard.
#include <hip/hip_runtime.h>

#include <cstring>

#include "bls_kernels.h"
#include "bls_keygen_batch.h"
#include "cbft_internal.h"

static_assert(CBFT_BLS_G2_BYTES == 65, "sizes");
static_assert(CBFT_BLS_KEYGEN_MAX_BATCH == BLS_KEYGEN_LAUNCH_MAX, "one launch per call");

// the fixed-base comb of g2, as cbft_bls_public_key builds it; complete before any stream reads it
static hipError_t keygen_table(cbft_ctx* c) {
  if (c->bls_pub_tbl.p) return hipSuccess;
  hipError_t e = c->bls_pub_tbl.reserve(cbft_bls_pub_table_words() * sizeof(uint32_t));
  if (e == hipSuccess) e = cbft_bls_launch_pub_table(c->bls_pub_tbl.as<uint32_t>(), c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) c->bls_pub_tbl.release();
  return e;
}

// after a call's launches, whatever happened: the device copies of its secrets are cleared, the stream
// drains, the staging is wiped
static hipError_t keygen_clear(cbft_ctx* c, void* d_secret, size_t bytes, hipError_t e) {
  if (d_secret && bytes) {
    const hipError_t e1 = hipMemsetAsync(d_secret, 0, bytes, c->stream);
    if (e == hipSuccess) e = e1;
  }
  const hipError_t e2 = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = e2;
  if (c->blsk.hin.p) cbft_wipe(c->blsk.hin.p, c->blsk.hin.cap);
  return e;
}

void cbft_bls_keygen_release(cbft_ctx* c) {
  (void)hipSetDevice(c->device);
  c->blsk.scratch.drain_and_zero(c->stream);
  if (c->blsk.in.p) (void)hipMemsetAsync(c->blsk.in.p, 0, c->blsk.in.cap, c->stream);
  (void)hipStreamSynchronize(c->stream);
  if (c->blsk.hin.p) cbft_wipe(c->blsk.hin.p, c->blsk.hin.cap);
  c->blsk.hin.release();
  for (DevBuf* b : {&c->blsk.in, &c->blsk.out}) b->release();
  c->blsk.scratch.release();
}

extern "C" {

int cbft_bls_public_key_batch(cbft_ctx* c, const uint8_t* sk32, size_t n, uint8_t* out65, uint8_t* ok) {
  c = cbft_dev0(c);
  if (!c || (n && (!sk32 || !out65 || !ok))) return CBFT_EINVAL;
  if (n == 0) return CBFT_OK;
  if (n > CBFT_BLS_KEYGEN_MAX_BATCH) return CBFT_E2BIG;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  const size_t kbytes = n * 32, obytes = n * CBFT_BLS_G2_BYTES;
  hipError_t e = keygen_table(c);
  if (e == hipSuccess) e = c->blsk.hin.reserve(kbytes);
  if (e == hipSuccess) e = c->blsk.in.reserve(kbytes);
  if (e == hipSuccess) e = c->blsk.out.reserve(obytes + n);
  if (e != hipSuccess) return cbft_fail(e, "BLS keygen buffers", __FILE__, __LINE__);
  uint8_t* d_out = c->blsk.out.as<uint8_t>();
  std::memcpy(c->blsk.hin.p, sk32, kbytes);
  e = hipMemcpyAsync(c->blsk.in.p, c->blsk.hin.p, kbytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = cbft_bls_keygen_launch(c->bls_pub_tbl.as<uint32_t>(), c->blsk.in.as<uint8_t>(), nullptr, (uint32_t)n, d_out,
                               d_out + obytes, c->stream);
  e = keygen_clear(c, c->blsk.in.p, kbytes, e);
  if (e != hipSuccess) return cbft_fail(e, "BLS key batch", __FILE__, __LINE__);
  CBFT_HIP(hipMemcpy(out65, d_out, obytes, hipMemcpyDeviceToHost));
  CBFT_HIP(hipMemcpy(ok, d_out + obytes, n, hipMemcpyDeviceToHost));
  return CBFT_OK;
}

int cbft_bls_public_key_fixed_device(cbft_ctx* c, const uint8_t* d_sk32, size_t n, uint8_t* d_out65, uint8_t* d_ok,
                                     void* stream) {
  if (c && !c->kids.empty()) return CBFT_EINVAL;  // device pointers belong to one GPU: use its own context
  if (!c || (n && (!d_sk32 || !d_out65 || !d_ok))) return CBFT_EINVAL;
  if (n == 0) return CBFT_OK;
  if (n > CBFT_BLS_KEYGEN_MAX_BATCH) return CBFT_E2BIG;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(keygen_table(c));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  CBFT_HIP(cbft_bls_keygen_launch(c->bls_pub_tbl.as<uint32_t>(), d_sk32, nullptr, (uint32_t)n, d_out65, d_ok, s));
  return CBFT_OK;
}

int cbft_bls_keygen_threshold(cbft_ctx* c, const uint8_t* coeff32, uint32_t k, uint32_t n, uint8_t* out_sk32,
                              uint8_t* out_vk65, uint8_t* out_pk65, uint8_t* out_ok) {
  c = cbft_dev0(c);
  if (!c || !coeff32 || !out_sk32 || !out_vk65 || !out_pk65 || !out_ok) return CBFT_EINVAL;
  if (k < 1 || k > n || n > 2048u /* VectorOfShares ids */) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  // scratch: coefficients (k x 32) | their Montgomery forms (k x 9 words) | scalars ((n + 1) x 32): all secret
  const size_t cbytes = (size_t)k * 32, mbytes = (size_t)k * BN_LIMBS * sizeof(uint32_t);
  const size_t sbytes = ((size_t)n + 1) * 32, bytes = cbytes + mbytes + sbytes;
  const size_t obytes = ((size_t)n + 1) * CBFT_BLS_G2_BYTES;
  hipError_t e = keygen_table(c);
  if (e == hipSuccess) e = c->blsk.hin.reserve(cbytes);
  if (e == hipSuccess) e = c->blsk.out.reserve(obytes + n + 1);
  if (e == hipSuccess) e = c->blsk.scratch.acquire(bytes, c->stream);
  if (e != hipSuccess) return cbft_fail(e, "BLS keygen buffers", __FILE__, __LINE__);
  uint8_t* d = c->blsk.scratch.buf.as<uint8_t>();
  uint8_t* d_sk = d + cbytes + mbytes;
  uint8_t* d_out = c->blsk.out.as<uint8_t>();
  std::memcpy(c->blsk.hin.p, coeff32, cbytes);
  e = hipMemcpyAsync(d, c->blsk.hin.p, cbytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = cbft_bls_keygen_launch_deal(d, k, n, reinterpret_cast<uint32_t*>(d + cbytes), d_sk, c->stream);
  if (e == hipSuccess)
    e = cbft_bls_keygen_launch(c->bls_pub_tbl.as<uint32_t>(), d_sk, nullptr, n + 1, d_out, d_out + obytes, c->stream);
  // the shares are the caller's: they leave before the scratch is cleared (stream order)
  if (e == hipSuccess) e = hipMemcpyAsync(out_sk32, d_sk + 32, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream);
  e = keygen_clear(c, d, bytes, e);
  const hipError_t e1 = c->blsk.scratch.commit(c->stream);
  if (e == hipSuccess) e = e1;
  if (e != hipSuccess) {
    cbft_wipe(out_sk32, (size_t)n * 32);
    return cbft_fail(e, "BLS threshold keygen", __FILE__, __LINE__);
  }
  CBFT_HIP(hipMemcpy(out_pk65, d_out, CBFT_BLS_G2_BYTES, hipMemcpyDeviceToHost));
  CBFT_HIP(hipMemcpy(out_vk65, d_out + CBFT_BLS_G2_BYTES, (size_t)n * CBFT_BLS_G2_BYTES, hipMemcpyDeviceToHost));
  CBFT_HIP(hipMemcpy(out_ok, d_out + obytes, (size_t)n + 1, hipMemcpyDeviceToHost));
  return CBFT_OK;
}

}  // extern "C"
