// libcbft_hipcrypto, Ed25519 signing half of the C ABI (include/cbft_hipcrypto.h).
//
// The batch form of the one signature per pre-executed request that the reference makes on the
// host (PreProcessReplyMsg.cpp:142-160, RequestProcessingState.cpp:110,236, PreProcessResultMsg.cpp:
// 83): a signer table is loaded once (scalar, prefix and public key derived on the GPU from the
// seeds) and every sign is a batch on the GPU (ed25519_sign.hip).
//
// Multi-GPU contexts: signer tables live on the lowest device (cbft_dev0) and the host-array calls
// run there, like the non-sharded BLS calls; the _device entry needs a single-GPU context.
//
// Secrets: seeds pass through pinned staging that is zeroed once they are on the device, the
// device copy of the seeds is cleared after the records are built, the nonce scratch is cleared
// by the finish kernel per batch and again with the records when a table is unloaded and at close.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cbft_internal.h"

static_assert(CBFT_ED25519_SIGNATURE_BYTES == 64 && CBFT_ED25519_PUBLIC_KEY_BYTES == 32, "sizes");

// memset the optimiser may not drop
static void wipe(void* p, size_t n) {
  volatile uint8_t* v = static_cast<volatile uint8_t*>(p);
  for (size_t i = 0; i < n; i++) v[i] = 0;
}

static int sign_launch_locked(cbft_ctx* c, SignerTable& st, const uint32_t* d_idx, const uint8_t* d_msg,
                              const uint64_t* d_off, const uint32_t* d_len, uint32_t fixed_len, size_t n,
                              uint8_t* d_sig, hipStream_t s) {
  CBFT_HIP(c->sign_scratch.reserve(cbft_ed25519_sign_scratch_words(n) * sizeof(uint32_t)));
  if (!c->sign_done) CBFT_HIP(hipEventCreateWithFlags(&c->sign_done, hipEventDisableTiming));
  if (c->sign_used) CBFT_HIP(hipStreamWaitEvent(s, c->sign_done, 0));  // scratch reuse across streams
  Ed25519SignBatch b{n, st.rec.as<uint32_t>(), st.nkeys, d_idx, d_msg, d_off, d_len, fixed_len};
  CBFT_HIP(cbft_ed25519_sign_launch(b, c->sign_table.as<uint32_t>(), c->sign_scratch.as<uint32_t>(), d_sig, s));
  CBFT_HIP(hipEventRecord(c->sign_done, s));
  c->sign_used = true;
  return CBFT_OK;
}

// every stream that may still touch the signing state has drained (device-path batches run on
// caller streams), then the secret buffers are overwritten
static void sign_clear_scratch(cbft_ctx* c) {
  (void)hipDeviceSynchronize();
  if (c->sign_scratch.p) (void)hipMemsetAsync(c->sign_scratch.p, 0, c->sign_scratch.cap, c->stream);
}

void cbft_sign_release(cbft_ctx* c) {
  (void)hipSetDevice(c->device);
  sign_clear_scratch(c);
  for (auto& kv : c->signer_tables)
    if (kv.second.rec.p) (void)hipMemsetAsync(kv.second.rec.p, 0, kv.second.rec.cap, c->stream);
  (void)hipStreamSynchronize(c->stream);
  for (auto& kv : c->signer_tables) kv.second.rec.release();
  c->signer_tables.clear();
  for (DevBuf* b : {&c->sign_table, &c->sign_scratch, &c->sign_in, &c->sign_out}) b->release();
  if (c->sign_done) (void)hipEventDestroy(c->sign_done);
  c->sign_done = nullptr;
  c->sign_used = false;
}

extern "C" {

int cbft_ed25519_load_signers(cbft_ctx* c, const uint8_t* seed, uint32_t nkeys, uint32_t* out_id) {
  c = cbft_dev0(c);
  if (!c || !seed || !out_id || nkeys == 0) return CBFT_EINVAL;
  if (nkeys > (1u << 20)) return CBFT_E2BIG;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  if (!c->sign_table.p) {
    CBFT_HIP(c->sign_table.reserve((size_t)CBFT_SIGN_TABLE_WORDS * sizeof(uint32_t)));
    hipError_t e = cbft_ed25519_sign_build_table(c->sign_table.as<uint32_t>(), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
      c->sign_table.release();
      return cbft_fail(e, "sign comb table", __FILE__, __LINE__);
    }
  }
  SignerTable st;
  st.nkeys = nkeys;
  const size_t sbytes = (size_t)nkeys * 32;
  CBFT_HIP(st.rec.reserve((size_t)nkeys * CBFT_SIGNER_WORDS * sizeof(uint32_t)));
  HostBuf hs;
  DevBuf ds;
  hipError_t e = hs.reserve(sbytes);
  if (e == hipSuccess) e = ds.reserve(sbytes);
  if (e == hipSuccess) {
    std::memcpy(hs.p, seed, sbytes);
    e = hipMemcpyAsync(ds.p, hs.p, sbytes, hipMemcpyHostToDevice, c->stream);
  }
  if (e == hipSuccess)
    e = cbft_ed25519_sign_launch_keys(ds.as<uint8_t>(), nkeys, c->sign_table.as<uint32_t>(), st.rec.as<uint32_t>(),
                                      c->stream);
  if (e == hipSuccess && ds.p) e = hipMemsetAsync(ds.p, 0, ds.cap, c->stream);
  const hipError_t e2 = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = e2;
  if (hs.p) wipe(hs.p, hs.cap);  // the seeds are on the device (or the load failed): none stay here
  hs.release();
  ds.release();
  if (e != hipSuccess) {
    if (st.rec.p) (void)hipMemset(st.rec.p, 0, st.rec.cap);
    st.rec.release();
    return cbft_fail(e, "signer records", __FILE__, __LINE__);
  }
  const uint32_t id = c->next_signer_id++;
  c->signer_tables.emplace(id, std::move(st));
  *out_id = id;
  return CBFT_OK;
}

int cbft_ed25519_signer_public_keys(cbft_ctx* c, uint32_t id, uint8_t* out_pk) {
  c = cbft_dev0(c);
  if (!c || !out_pk) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->signer_tables.find(id);
  if (it == c->signer_tables.end()) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  // only the A part of each record crosses to the host
  CBFT_HIP(hipMemcpy2D(out_pk, 32, it->second.rec.as<uint32_t>() + 16, CBFT_SIGNER_WORDS * sizeof(uint32_t), 32,
                       it->second.nkeys, hipMemcpyDeviceToHost));
  return CBFT_OK;
}

int cbft_ed25519_unload_signers(cbft_ctx* c, uint32_t id) {
  c = cbft_dev0(c);
  if (!c) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->signer_tables.find(id);
  if (it == c->signer_tables.end()) return CBFT_EINVAL;
  (void)hipSetDevice(c->device);
  sign_clear_scratch(c);  // synchronises the device first: in-flight device-path batches read the table
  (void)hipMemsetAsync(it->second.rec.p, 0, it->second.rec.cap, c->stream);
  (void)hipStreamSynchronize(c->stream);
  it->second.rec.release();
  c->signer_tables.erase(it);
  return CBFT_OK;
}

int cbft_ed25519_sign_batch(cbft_ctx* c, uint32_t id, const uint32_t* signer_idx, const uint8_t* msg_blob,
                            const uint64_t* msg_off, const uint32_t* msg_len, size_t n, uint8_t* out_sig) {
  c = cbft_dev0(c);
  if (!c || (n && (!msg_off || !msg_len || !out_sig))) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->signer_tables.find(id);
  if (it == c->signer_tables.end()) return CBFT_EINVAL;
  if (n == 0) return CBFT_OK;
  // the batch's messages are the blob range [lo, hi) its offsets span: only that range moves
  uint64_t lo = UINT64_MAX, hi = 0;
  for (size_t i = 0; i < n; i++) {
    if (signer_idx && signer_idx[i] >= it->second.nkeys) return CBFT_EINVAL;
    if (msg_len[i] > CBFT_MAX_MSG_LEN) return CBFT_EINVAL;
    lo = std::min<uint64_t>(lo, msg_off[i]);
    hi = std::max<uint64_t>(hi, msg_off[i] + msg_len[i]);
  }
  if (hi > lo && !msg_blob) return CBFT_EINVAL;
  const uint64_t blob = hi > lo ? hi - lo : 0;
  // one packed device image: offsets (rebased) | lengths | signer indices | blob
  const size_t o_off = 0, o_len = n * 8, o_idx = o_len + n * 4, o_blob = o_idx + n * 4;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(c->sign_in.reserve(o_blob + blob + 16));
  CBFT_HIP(c->sign_out.reserve(n * 64));
  c->host_off.resize(n);
  for (size_t i = 0; i < n; i++) c->host_off[i] = msg_off[i] - lo;
  uint8_t* d = c->sign_in.as<uint8_t>();
  CBFT_HIP(hipMemcpyAsync(d + o_off, c->host_off.data(), n * 8, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(hipMemcpyAsync(d + o_len, msg_len, n * 4, hipMemcpyHostToDevice, c->stream));
  if (signer_idx) CBFT_HIP(hipMemcpyAsync(d + o_idx, signer_idx, n * 4, hipMemcpyHostToDevice, c->stream));
  if (blob) CBFT_HIP(hipMemcpyAsync(d + o_blob, msg_blob + lo, blob, hipMemcpyHostToDevice, c->stream));
  const int rc = sign_launch_locked(c, it->second, signer_idx ? reinterpret_cast<const uint32_t*>(d + o_idx) : nullptr,
                                    d + o_blob, reinterpret_cast<const uint64_t*>(d + o_off),
                                    reinterpret_cast<const uint32_t*>(d + o_len), 0, n, c->sign_out.as<uint8_t>(),
                                    c->stream);
  if (rc) return rc;
  CBFT_HIP(hipMemcpyAsync(out_sig, c->sign_out.p, n * 64, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  return CBFT_OK;
}

int cbft_ed25519_sign_fixed_device(cbft_ctx* c, uint32_t id, const uint32_t* d_signer_idx, const uint8_t* d_msg,
                                   uint32_t msg_len, size_t n, uint8_t* d_sig, void* stream) {
  if (c && !c->kids.empty()) return CBFT_EINVAL;  // device pointers belong to one GPU: use its own context
  if (!c || (n && (!d_sig || (msg_len && !d_msg)))) return CBFT_EINVAL;
  if (msg_len > CBFT_MAX_MSG_LEN) return CBFT_EINVAL;
  if (reinterpret_cast<uintptr_t>(d_sig) & 3) return CBFT_EINVAL;  // signatures are written as words
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->signer_tables.find(id);
  if (it == c->signer_tables.end()) return CBFT_EINVAL;
  if (n == 0) return CBFT_OK;
  CBFT_HIP(hipSetDevice(c->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  return sign_launch_locked(c, it->second, d_signer_idx, d_msg, nullptr, nullptr, msg_len, n, d_sig, s);
}

}  // extern "C"
