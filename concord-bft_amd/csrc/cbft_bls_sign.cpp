// libcbft_hipcrypto, batched BLS share signing half of the C ABI (include/cbft_hipcrypto.h).
//
// The batch form of IThresholdSigner::signData: a replica signs at least two shares per sequence
// number (SignedShareBase::create, SignedShareMsgs.cpp:57; PartialCommitProofMsg.cpp:44) with one of
// a few threshold signers, and many sequence numbers are in flight.  A signer table is loaded once
// (per signer: the GLV halves of the scalar, recoded; bls_sign_batch.h) and every sign is a batch with
// one message per lane (bls_sign_batch.hip).  cbft_bls_sign stays the one-message call.
//
// Multi-GPU contexts: signer tables live on the lowest device (cbft_dev0) and the host-array calls
// run there, like RSA signing; the _device entry needs a single-GPU context.
//
// Secrets: the scalars pass through pinned staging that is zeroed once they are on the device, the
// device copy is cleared after the records (and the public keys) are built, and the records are
// cleared when a table is unloaded and at close.  The batch scratch holds public values only (the
// hash points; their odd multiples live in LDS); it is cleared with the records all the same.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "bls_kernels.h"
#include "bls_keygen_batch.h"
#include "bls_sign_batch.h"
#include "cbft_internal.h"

static_assert(CBFT_BLS_SHARE_BYTES == 37 && CBFT_BLS_G2_BYTES == 65, "sizes");

static int bls_sign_launch_locked(cbft_ctx* c, BlsSignerTable& st, const uint32_t* d_idx, const uint8_t* d_msg,
                                  const uint64_t* d_off, const uint32_t* d_len, uint32_t fixed_len, size_t n,
                                  uint8_t* d_out, hipStream_t s) {
  CBFT_HIP(c->blss.scratch.acquire(cbft_bls_sign_scratch_words(n) * sizeof(uint32_t), s));
  BlsSignBatch b{n, st.rec.as<uint32_t>(), st.nkeys, d_idx, d_msg, d_off, d_len, fixed_len};
  CBFT_HIP(cbft_bls_sign_launch(b, c->blss.scratch.buf.as<uint32_t>(), d_out, nullptr, s));
  CBFT_HIP(c->blss.scratch.commit(s));
  return CBFT_OK;
}

static void bls_sign_drop_table(cbft_ctx* c, BlsSignerTable& st) {
  cbft_clear_release(st.rec, c->stream);
  st.vk65.release();
}

void cbft_bls_sign_release(cbft_ctx* c) {
  (void)hipSetDevice(c->device);
  c->blss.scratch.drain_and_zero(c->stream);
  for (auto& kv : c->bls_signer_tables) bls_sign_drop_table(c, kv.second);
  (void)hipStreamSynchronize(c->stream);
  c->bls_signer_tables.clear();
  for (DevBuf* b : {&c->blss.in, &c->blss.out}) b->release();
  c->blss.scratch.release();
}

extern "C" {

int cbft_bls_load_signers(cbft_ctx* c, const uint8_t* sk32, const uint32_t* ids, uint32_t nkeys, uint32_t* out_id) {
  c = cbft_dev0(c);
  if (!c || !sk32 || !ids || !out_id || nkeys == 0) return CBFT_EINVAL;
  if (nkeys > (1u << 16)) return CBFT_E2BIG;
  for (uint32_t i = 0; i < nkeys; i++)
    if (ids[i] < 1 || ids[i] > 2048u  /* VectorOfShares ids */) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  // staging image: nkeys x 8 scalar words | nkeys ids
  const size_t kbytes = (size_t)nkeys * 32, bytes = kbytes + (size_t)nkeys * 4;
  HostBuf hs;
  DevBuf ds;
  BlsSignerTable st;
  st.nkeys = nkeys;
  hipError_t e = hs.reserve(bytes);
  bool valid = true;
  if (e == hipSuccess) {
    for (uint32_t i = 0; i < nkeys && valid; i++) valid = cbft_bls_scalar_words(hs.as<uint32_t>() + 8 * (size_t)i, sk32 + 32 * (size_t)i);
    std::memcpy(hs.as<uint8_t>(kbytes), ids, (size_t)nkeys * 4);
  }
  if (e != hipSuccess || !valid) {
    if (hs.p) cbft_wipe(hs.p, hs.cap);
    hs.release();
    return e != hipSuccess ? cbft_fail(e, "signer staging", __FILE__, __LINE__) : CBFT_EINVAL;
  }
  e = ds.reserve(bytes);
  if (e == hipSuccess) e = st.rec.reserve((size_t)nkeys * BLS_SIGNER_WORDS * sizeof(uint32_t));
  if (e == hipSuccess) e = st.vk65.reserve((size_t)nkeys * CBFT_BLS_G2_BYTES);
  if (e == hipSuccess && !c->bls_pub_tbl.p) {  // fixed-base comb of g2, as cbft_bls_public_key builds it
    e = c->bls_pub_tbl.reserve(cbft_bls_pub_table_words() * sizeof(uint32_t));
    if (e == hipSuccess) e = cbft_bls_launch_pub_table(c->bls_pub_tbl.as<uint32_t>(), c->stream);
    if (e != hipSuccess) c->bls_pub_tbl.release();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(ds.p, hs.p, bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = cbft_bls_sign_launch_keys(ds.as<uint32_t>(), ds.as<uint32_t>() + 8 * (size_t)nkeys, nkeys, st.rec.as<uint32_t>(),
                                  c->stream);
  // vk_i = sk_i * g2: one key per lane from the measured crossover on (bls_keygen_batch.h), else a launch per key
  const bool batch = nkeys >= CBFT_BLS_KEYGEN_BATCH_MIN_DEFAULT;
  if (e == hipSuccess && batch)
    e = cbft_bls_keygen_launch(c->bls_pub_tbl.as<uint32_t>(), nullptr, ds.as<uint32_t>(), nkeys, st.vk65.as<uint8_t>(),
                               nullptr, c->stream);
  for (uint32_t i = 0; i < nkeys && !batch && e == hipSuccess; i++)
    e = cbft_bls_launch_pubkey_row(c->bls_pub_tbl.as<uint32_t>(), ds.as<uint32_t>() + 8 * (size_t)i,
                                   st.vk65.as<uint8_t>() + CBFT_BLS_G2_BYTES * (size_t)i, c->stream);
  if (ds.p) {  // the scalars leave the device, whatever happened
    const hipError_t e1 = hipMemsetAsync(ds.p, 0, ds.cap, c->stream);
    if (e == hipSuccess) e = e1;
  }
  const hipError_t e2 = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = e2;
  cbft_wipe(hs.p, hs.cap);  // the scalars are on the device (or the load failed): none stay here
  hs.release();
  ds.release();
  if (e != hipSuccess) {
    bls_sign_drop_table(c, st);
    return cbft_fail(e, "BLS signer records", __FILE__, __LINE__);
  }
  const uint32_t id = c->next_bls_signer_id++;
  c->bls_signer_tables.emplace(id, std::move(st));
  *out_id = id;
  return CBFT_OK;
}

int cbft_bls_signer_public_keys(cbft_ctx* c, uint32_t id, uint8_t* out65) {
  c = cbft_dev0(c);
  if (!c || !out65) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->bls_signer_tables.find(id);
  if (it == c->bls_signer_tables.end()) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(hipMemcpy(out65, it->second.vk65.p, (size_t)it->second.nkeys * CBFT_BLS_G2_BYTES, hipMemcpyDeviceToHost));
  return CBFT_OK;
}

int cbft_bls_unload_signers(cbft_ctx* c, uint32_t id) {
  c = cbft_dev0(c);
  if (!c) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->bls_signer_tables.find(id);
  if (it == c->bls_signer_tables.end()) return CBFT_EINVAL;
  (void)hipSetDevice(c->device);
  // synchronises the device first: in-flight device-path batches read the table
  c->blss.scratch.drain_and_zero(c->stream);
  bls_sign_drop_table(c, it->second);
  c->bls_signer_tables.erase(it);
  return CBFT_OK;
}

int cbft_bls_sign_batch(cbft_ctx* c, uint32_t id, const uint32_t* signer_idx, const uint8_t* msg_blob,
                        const uint64_t* msg_off, const uint32_t* msg_len, size_t n, uint8_t* out37) {
  c = cbft_dev0(c);
  if (!c || (n && (!msg_off || !msg_len || !out37))) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->bls_signer_tables.find(id);
  if (it == c->bls_signer_tables.end()) return CBFT_EINVAL;
  if (n == 0) return CBFT_OK;
  for (size_t i = 0; i < n; i++)
    if (signer_idx && signer_idx[i] >= it->second.nkeys) return CBFT_EINVAL;
  c->host_off.resize(n);
  const CbftSpan span = cbft_msg_span(msg_off, msg_len, n, CBFT_MAX_MSG_LEN, msg_blob != nullptr, c->host_off.data());
  if (span.err) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  const CbftPackedArray idx{signer_idx, n * 4};
  CbftPackedLayout L;
  CBFT_HIP(cbft_upload_packed(c->blss.in, c->stream, c->host_off.data(), msg_len, n, &idx, 1, msg_blob, span, &L));
  CBFT_HIP(c->blss.out.reserve(n * CBFT_BLS_SHARE_BYTES));
  const uint8_t* d = c->blss.in.as<uint8_t>();
  const int rc = bls_sign_launch_locked(c, it->second, signer_idx ? reinterpret_cast<const uint32_t*>(d + L.mid[0]) : nullptr,
                                        d + L.blob, reinterpret_cast<const uint64_t*>(d + L.off),
                                        reinterpret_cast<const uint32_t*>(d + L.len), 0, n, c->blss.out.as<uint8_t>(),
                                        c->stream);
  if (rc) return rc;
  CBFT_HIP(hipMemcpyAsync(out37, c->blss.out.p, n * CBFT_BLS_SHARE_BYTES, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  return CBFT_OK;
}

int cbft_bls_sign_fixed_device(cbft_ctx* c, uint32_t id, const uint32_t* d_signer_idx, const uint8_t* d_msg,
                               uint32_t msg_len, size_t n, uint8_t* d_out37, void* stream) {
  if (c && !c->kids.empty()) return CBFT_EINVAL;  // device pointers belong to one GPU: use its own context
  if (!c || (n && (!d_out37 || (msg_len && !d_msg)))) return CBFT_EINVAL;
  if (msg_len > CBFT_MAX_MSG_LEN) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->bls_signer_tables.find(id);
  if (it == c->bls_signer_tables.end()) return CBFT_EINVAL;
  if (n == 0) return CBFT_OK;
  CBFT_HIP(hipSetDevice(c->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  return bls_sign_launch_locked(c, it->second, d_signer_idx, d_msg, nullptr, nullptr, msg_len, n, d_out37, s);
}

}  // extern "C"
