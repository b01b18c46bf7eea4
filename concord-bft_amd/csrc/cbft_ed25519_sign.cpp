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

#include <cstdlib>
#include <cstring>
#include <vector>

#include "cbft_internal.h"

static_assert(CBFT_ED25519_SIGNATURE_BYTES == 64 && CBFT_ED25519_PUBLIC_KEY_BYTES == 32, "sizes");

static int sign_launch_locked(cbft_ctx* c, SignerTable& st, const uint32_t* d_idx, const uint8_t* d_msg,
                              const uint64_t* d_off, const uint32_t* d_len, uint32_t fixed_len, size_t n,
                              uint8_t* d_sig, hipStream_t s) {
  CBFT_HIP(c->sign.scratch.acquire(cbft_ed25519_sign_scratch_words(n) * sizeof(uint32_t), s));
  Ed25519SignBatch b{n, st.rec.as<uint32_t>(), st.nkeys, d_idx, d_msg, d_off, d_len, fixed_len};
  CBFT_HIP(cbft_ed25519_sign_launch(b, c->sign.table.as<uint32_t>(), c->sign.scratch.buf.as<uint32_t>(), d_sig, s));
  CBFT_HIP(c->sign.scratch.commit(s));
  return CBFT_OK;
}

void cbft_sign_release(cbft_ctx* c) {
  (void)hipSetDevice(c->device);
  c->sign.scratch.drain_and_zero(c->stream);
  for (auto& kv : c->signer_tables) cbft_clear_release(kv.second.rec, c->stream);
  (void)hipStreamSynchronize(c->stream);
  c->signer_tables.clear();
  for (DevBuf* b : {&c->sign.table, &c->sign.in, &c->sign.out}) b->release();
  c->sign.scratch.release();
}

extern "C" {

int cbft_ed25519_load_signers(cbft_ctx* c, const uint8_t* seed, uint32_t nkeys, uint32_t* out_id) {
  c = cbft_dev0(c);
  if (!c || !seed || !out_id || nkeys == 0) return CBFT_EINVAL;
  if (nkeys > (1u << 20)) return CBFT_E2BIG;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  if (!c->sign.table.p) {
    CBFT_HIP(c->sign.table.reserve((size_t)CBFT_SIGN_TABLE_WORDS * sizeof(uint32_t)));
    hipError_t e = cbft_ed25519_sign_build_table(c->sign.table.as<uint32_t>(), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
      c->sign.table.release();
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
    e = cbft_ed25519_sign_launch_keys(ds.as<uint8_t>(), nkeys, c->sign.table.as<uint32_t>(), st.rec.as<uint32_t>(),
                                      c->stream);
  if (e == hipSuccess && ds.p) e = hipMemsetAsync(ds.p, 0, ds.cap, c->stream);
  const hipError_t e2 = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = e2;
  if (hs.p) cbft_wipe(hs.p, hs.cap);  // the seeds are on the device (or the load failed): none stay here
  hs.release();
  ds.release();
  if (e != hipSuccess) {
    cbft_clear_release(st.rec, c->stream);
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
  // synchronises the device first: in-flight device-path batches read the table
  c->sign.scratch.drain_and_zero(c->stream);
  cbft_clear_release(it->second.rec, c->stream);
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
  for (size_t i = 0; i < n; i++)
    if (signer_idx && signer_idx[i] >= it->second.nkeys) return CBFT_EINVAL;
  c->host_off.resize(n);
  const CbftSpan span = cbft_msg_span(msg_off, msg_len, n, CBFT_MAX_MSG_LEN, msg_blob != nullptr, c->host_off.data());
  if (span.err) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  const CbftPackedArray idx{signer_idx, n * 4};
  CbftPackedLayout L;
  CBFT_HIP(cbft_upload_packed(c->sign.in, c->stream, c->host_off.data(), msg_len, n, &idx, 1, msg_blob, span, &L));
  CBFT_HIP(c->sign.out.reserve(n * 64));
  const uint8_t* d = c->sign.in.as<uint8_t>();
  const int rc = sign_launch_locked(c, it->second, signer_idx ? reinterpret_cast<const uint32_t*>(d + L.mid[0]) : nullptr,
                                    d + L.blob, reinterpret_cast<const uint64_t*>(d + L.off),
                                    reinterpret_cast<const uint32_t*>(d + L.len), 0, n, c->sign.out.as<uint8_t>(),
                                    c->stream);
  if (rc) return rc;
  CBFT_HIP(hipMemcpyAsync(out_sig, c->sign.out.p, n * 64, hipMemcpyDeviceToHost, c->stream));
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
