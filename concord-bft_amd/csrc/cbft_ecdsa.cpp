// libcbft_hipcrypto, ECDSA secp256k1 / SHA-256 half of the C ABI (include/cbft_hipcrypto.h), and P-256 /
// SHA-256 verification behind the same calls: a key table remembers its curve (cbft_ecdsa_load_keys_curve),
// ids share one space, and every other call dispatches on the table's curve.
//
// Replaces concord::util::crypto::ECDSAVerifier (util/src/crypto_utils.cpp:34-64,231-236): one
// verifier per key there; here a key table is loaded once (keys validated and their window tables
// built on the GPU) and every verify is a batch on the GPU.
//
// Multi-GPU contexts: key tables are loaded on every device (table ids in step) and a host-buffer
// batch is cut into contiguous shards of whole 64-signature verdict words, one per device, as for
// RSA.  The _device entry point needs a single-GPU context (CBFT_EINVAL otherwise).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "cbft_internal.h"
#include "ecdsa_p256_verify.h"
#include "ecdsa_verify.h"

static_assert(CBFT_ECDSA_PUBLIC_KEY_BYTES == ECDSA_PUB_BYTES, "key size");
static_assert(CBFT_ECDSA_SIGNATURE_BYTES == ECDSA_SIG_BYTES, "signature size");

void cbft_ecdsa_release(cbft_ctx* c) {
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();  // device-path batches run on caller streams
  for (auto& kv : c->ecdsa_tables) kv.second.rec.release();
  c->ecdsa_tables.clear();
  for (DevBuf* b : {&c->ecdsa.gtab, &c->ecdsa.gtab_p256, &c->ecdsa.sig, &c->ecdsa.kidx}) b->release();
  c->ecdsa.scratch.release();
  c->ecdsa.timer.release();
}

static hipError_t ecdsa_launch_keys(int curve, const uint8_t* d_pub, uint32_t nkeys, uint32_t* d_keys, hipStream_t s) {
  return curve == CBFT_CURVE_P256 ? cbft_ecdsa_p256_launch_keys(d_pub, nkeys, d_keys, s)
                                  : cbft_ecdsa_launch_keys(d_pub, nkeys, d_keys, s);
}

// G's window table: the record of the key Q = G, built once per context and curve by the key-load kernel
static int ecdsa_gtab_locked(cbft_ctx* c, int curve) {
  DevBuf& slot = curve == CBFT_CURVE_P256 ? c->ecdsa.gtab_p256 : c->ecdsa.gtab;
  if (slot.p) return CBFT_OK;
  static const uint8_t g_k1[ECDSA_PUB_BYTES] = ECDSA_G_BYTES;
  static const uint8_t g_p256[ECDSA_PUB_BYTES] = ECDSA_P256_G_BYTES;
  const uint8_t* g = curve == CBFT_CURVE_P256 ? g_p256 : g_k1;
  DevBuf pub, tab;
  hipError_t e = pub.reserve(ECDSA_PUB_BYTES);
  if (e == hipSuccess) e = tab.reserve(ECDSA_KEY_WORDS * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpyAsync(pub.p, g, ECDSA_PUB_BYTES, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = ecdsa_launch_keys(curve, pub.as<uint8_t>(), 1, tab.as<uint32_t>(), c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  pub.release();
  if (e != hipSuccess) {
    tab.release();
    return cbft_fail(e, "ecdsa generator table", __FILE__, __LINE__);
  }
  slot = tab;
  return CBFT_OK;
}

static int ecdsa_launch_locked(cbft_ctx* c, EcdsaKeyTable& kt, const uint32_t* d_kidx, const uint8_t* d_sig,
                               const uint8_t* d_msg, const uint64_t* d_off, const uint32_t* d_len, size_t n,
                               uint64_t* d_verdicts, hipStream_t s) {
  CBFT_HIP(c->ecdsa.scratch.acquire(cbft_ecdsa_scratch_words(n) * sizeof(uint32_t), s));
  const bool p256 = kt.curve == CBFT_CURVE_P256;
  const DevBuf& gtab = p256 ? c->ecdsa.gtab_p256 : c->ecdsa.gtab;
  EcdsaBatch b{n, kt.rec.as<uint32_t>(), kt.nkeys, gtab.as<uint32_t>(), d_kidx, d_sig, d_msg, d_off, d_len};
  CBFT_HIP(c->ecdsa.timer.begin(c->profiling, s));
  if (p256)
    CBFT_HIP(cbft_ecdsa_p256_launch_verify(b, c->ecdsa.scratch.buf.as<uint32_t>(), d_verdicts, s));
  else
    CBFT_HIP(cbft_ecdsa_launch_verify(b, c->ecdsa.scratch.buf.as<uint32_t>(), d_verdicts, s));
  CBFT_HIP(c->ecdsa.timer.end(c->profiling, s));
  CBFT_HIP(c->ecdsa.scratch.commit(s));
  return CBFT_OK;
}

extern "C" {

// One device's key records under `want_id` (chosen by a multi-device parent, so every device
// holds the table under the same id) or under the device's next id when want_id == 0.
static int ecdsa_load_on(cbft_ctx* c, int curve, const uint8_t* pub, uint32_t nkeys, uint32_t want_id,
                         uint32_t* out_id) {
  std::lock_guard<std::mutex> g(c->mu);
  if (want_id && c->ecdsa_tables.count(want_id)) return CBFT_EIO;
  CBFT_HIP(hipSetDevice(c->device));
  const int grc = ecdsa_gtab_locked(c, curve);
  if (grc) return grc;
  EcdsaKeyTable kt;
  kt.nkeys = nkeys;
  kt.curve = curve;
  const size_t nk = std::max<uint32_t>(nkeys, 1);
  CBFT_HIP(kt.rec.reserve(nk * ECDSA_KEY_WORDS * sizeof(uint32_t)));
  if (nkeys) {
    DevBuf in;
    hipError_t e = in.reserve((size_t)nkeys * ECDSA_PUB_BYTES);
    if (e == hipSuccess) e = hipMemcpyAsync(in.p, pub, (size_t)nkeys * ECDSA_PUB_BYTES, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = ecdsa_launch_keys(curve, in.as<uint8_t>(), nkeys, kt.rec.as<uint32_t>(), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    in.release();
    if (e != hipSuccess) {
      kt.rec.release();
      return cbft_fail(e, "ecdsa key records", __FILE__, __LINE__);
    }
  }
  const uint32_t id = want_id ? want_id : c->next_ecdsa_id++;
  c->ecdsa_tables.emplace(id, std::move(kt));
  *out_id = id;
  return CBFT_OK;
}

int cbft_ecdsa_load_keys(cbft_ctx* c, const uint8_t* pub, uint32_t nkeys, uint32_t* out_id) {
  return cbft_ecdsa_load_keys_curve(c, CBFT_CURVE_SECP256K1, pub, nkeys, out_id);
}

int cbft_ecdsa_load_keys_curve(cbft_ctx* c, int curve, const uint8_t* pub, uint32_t nkeys, uint32_t* out_id) {
  if (!c || !out_id || (nkeys && !pub)) return CBFT_EINVAL;
  if (curve != CBFT_CURVE_SECP256K1 && curve != CBFT_CURVE_P256) return CBFT_EINVAL;
  if (nkeys > CBFT_ECDSA_MAX_KEYS) return CBFT_E2BIG;
  if (c->kids.empty()) return ecdsa_load_on(c, curve, pub, nkeys, 0, out_id);
  // every device, concurrently, under one id the parent allocates; a device that failed leaves
  // no table behind on the others (they unload theirs), so ids stay in step for later loads
  uint32_t id;
  {
    std::lock_guard<std::mutex> g(c->mu);
    id = c->next_ecdsa_id++;
  }
  std::vector<int> rcs(c->kids.size(), CBFT_OK);
  (void)for_each_kid(c, [&](size_t g) {
    uint32_t got = 0;
    return rcs[g] = ecdsa_load_on(c->kids[g], curve, pub, nkeys, id, &got);
  });
  int rc = CBFT_OK;
  for (int r : rcs)
    if (r && !rc) rc = r;
  if (rc) {
    for (size_t g = 0; g < c->kids.size(); g++)
      if (rcs[g] == CBFT_OK) (void)cbft_ecdsa_unload_keys(c->kids[g], id);
    return rc;
  }
  *out_id = id;
  return CBFT_OK;
}

int cbft_ecdsa_unload_keys(cbft_ctx* c, uint32_t id) {
  if (!c) return CBFT_EINVAL;
  if (!c->kids.empty()) {
    int rc = CBFT_OK;
    for (cbft_ctx* k : c->kids) {
      const int r = cbft_ecdsa_unload_keys(k, id);
      if (r && !rc) rc = r;
    }
    return rc;
  }
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->ecdsa_tables.find(id);
  if (it == c->ecdsa_tables.end()) return CBFT_EINVAL;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();  // in-flight device-path batches on caller streams read it
  it->second.rec.release();
  c->ecdsa_tables.erase(it);
  return CBFT_OK;
}

int cbft_ecdsa_key_status(cbft_ctx* c, uint32_t id, uint8_t* out_ok) {
  c = cbft_dev0(c);
  if (!c || !out_ok) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->ecdsa_tables.find(id);
  if (it == c->ecdsa_tables.end()) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  const uint32_t nkeys = it->second.nkeys;
  std::vector<uint32_t> ok(nkeys);
  if (nkeys)  // the validity word of every record: one strided copy
    CBFT_HIP(hipMemcpy2D(ok.data(), sizeof(uint32_t), it->second.rec.as<uint32_t>() + ECDSA_KEY_OK,
                         ECDSA_KEY_WORDS * sizeof(uint32_t), sizeof(uint32_t), nkeys, hipMemcpyDeviceToHost));
  for (uint32_t k = 0; k < nkeys; k++) out_ok[k] = ok[k] ? 1 : 0;
  return CBFT_OK;
}

int cbft_ecdsa_verify_batch(cbft_ctx* c, uint32_t id, const uint32_t* key_idx, const uint8_t* sig,
                            const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len, size_t n,
                            uint8_t* bitmap) {
  if (!c) return CBFT_EINVAL;
  if (n > CBFT_ECDSA_MAX_BATCH) return CBFT_E2BIG;
  if (n && (!key_idx || !sig || !msg_off || !msg_len || !bitmap)) return CBFT_EINVAL;
  if (n == 0) return CBFT_OK;
  if (!c->kids.empty()) {  // contiguous shards of whole 64-signature words, one per device
    const size_t G = c->kids.size();
    const size_t per = (((n + G - 1) / G) + 63) / 64 * 64;
    return for_each_kid(c, [&](size_t g) {
      const size_t lo = g * per;
      if (lo >= n) return (int)CBFT_OK;
      const size_t m = std::min(n, lo + per) - lo;
      return cbft_ecdsa_verify_batch(c->kids[g], id, key_idx + lo, sig + lo * ECDSA_SIG_BYTES, msg_blob, msg_off + lo,
                                     msg_len + lo, m, bitmap + lo / 8);
    });
  }
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->ecdsa_tables.find(id);
  if (it == c->ecdsa_tables.end()) return CBFT_EINVAL;
  for (size_t i = 0; i < n; i++)
    if (key_idx[i] >= it->second.nkeys) return CBFT_EINVAL;
  // no cap on a message's length: SHA-256 takes any
  c->host_off.resize(n);
  const CbftSpan span = cbft_msg_span(msg_off, msg_len, n, 0, msg_blob != nullptr, c->host_off.data());
  if (span.err) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(c->ecdsa.kidx.reserve(n * 4));
  CBFT_HIP(c->ecdsa.sig.reserve(n * ECDSA_SIG_BYTES));
  CBFT_HIP(c->msg.reserve(span.blob + 16));
  CBFT_HIP(c->off.reserve(n * 8));
  CBFT_HIP(c->len.reserve(n * 4));
  CBFT_HIP(c->verdicts.reserve(((n + 63) / 64) * 8));
  CBFT_HIP(hipMemcpyAsync(c->ecdsa.kidx.p, key_idx, n * 4, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(hipMemcpyAsync(c->ecdsa.sig.p, sig, n * ECDSA_SIG_BYTES, hipMemcpyHostToDevice, c->stream));
  if (span.blob) CBFT_HIP(hipMemcpyAsync(c->msg.p, msg_blob + span.lo, span.blob, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(hipMemcpyAsync(c->off.p, c->host_off.data(), n * 8, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(hipMemcpyAsync(c->len.p, msg_len, n * 4, hipMemcpyHostToDevice, c->stream));
  int rc = ecdsa_launch_locked(c, it->second, c->ecdsa.kidx.as<uint32_t>(), c->ecdsa.sig.as<uint8_t>(),
                               c->msg.as<uint8_t>(), c->off.as<uint64_t>(), c->len.as<uint32_t>(), n,
                               c->verdicts.as<uint64_t>(), c->stream);
  if (rc) return rc;
  return cbft_fetch_bitmap(c, n, bitmap);
}

int cbft_ecdsa_verify_batch_device(cbft_ctx* c, uint32_t id, const uint32_t* d_key_idx, const uint8_t* d_sig,
                                   const uint8_t* d_msg, const uint64_t* d_off, const uint32_t* d_len, size_t n,
                                   uint64_t* d_verdicts, void* stream) {
  if (c && !c->kids.empty()) return CBFT_EINVAL;  // device pointers belong to one GPU: use its own context
  if (!c) return CBFT_EINVAL;
  if (n > CBFT_ECDSA_MAX_BATCH) return CBFT_E2BIG;
  if (n && (!d_key_idx || !d_sig || !d_off || !d_len || !d_verdicts)) return CBFT_EINVAL;
  if (n == 0) return CBFT_OK;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->ecdsa_tables.find(id);
  if (it == c->ecdsa_tables.end()) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  return ecdsa_launch_locked(c, it->second, d_key_idx, d_sig, d_msg, d_off, d_len, n, d_verdicts, s);
}

int cbft_ecdsa_kernel_ms(cbft_ctx* c, float* out_ms) {
  c = cbft_dev0(c);
  if (!c || !out_ms) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->ecdsa.timer.valid) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(c->ecdsa.timer.elapsed(out_ms));
  return CBFT_OK;
}

}  // extern "C"
