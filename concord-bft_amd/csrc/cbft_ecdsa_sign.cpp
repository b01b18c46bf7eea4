// libcbft_hipcrypto, ECDSA signing half of the C ABI (include/cbft_hipcrypto.h).
//
// The batch form of concord::util::crypto::ECDSASigner (util/src/crypto_utils.cpp:66-99, secp256k1)
// and of concord::util::openssl_utils::AsymmetricPrivateKey::sign (util/src/openssl_crypto.cpp,
// P-256): a signer table is loaded once (range check and public key x G on the GPU) and every sign
// is a batch on the GPU (ecdsa_sign.hip, ecdsa_p256_sign.hip), with RFC 6979 nonces.  A table
// remembers its curve and every later call dispatches on it; each curve has its own comb table.
//
// Multi-GPU contexts: signer tables live on the lowest device (cbft_dev0) and the host-array calls
// run there, like Ed25519 signing; the _device entry needs a single-GPU context.
//
// Secrets: private keys pass through pinned staging that is wiped once they are on the device, the
// device copy of the raw keys is cleared after the records are built, and the records are zeroed
// when a table is unloaded and at close.  A batch's nonces cross one launch boundary in the context's
// scratch (a ScratchGuard orders batches on different streams): the point kernel zeroes them as it
// reads them, and the scratch is zeroed again at unload and at close.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "cbft_internal.h"
#include "ecdsa_p256_sign.h"
#include "ecdsa_sign.h"

static_assert(CBFT_ECDSA_PRIVATE_KEY_BYTES == ECDSAS_PRIV_BYTES, "key size");

static int ecdsas_launch_locked(cbft_ctx* c, EcdsaSignerTable& st, const uint32_t* d_idx, const uint8_t* d_msg,
                                const uint64_t* d_off, const uint32_t* d_len, uint32_t fixed_len, size_t n,
                                uint8_t* d_sig, hipStream_t s) {
  CBFT_HIP(c->ecdsas.scratch.acquire(cbft_ecdsa_sign_scratch_words(n) * sizeof(uint32_t), s));
  EcdsaSignBatch b{n, st.rec.as<uint32_t>(), st.nkeys, d_idx, d_msg, d_off, d_len, fixed_len};
  CBFT_HIP(c->ecdsas.timer.begin(c->profiling, s));
  if (st.curve == CBFT_CURVE_P256) {
    CBFT_HIP(cbft_ecdsa_p256_sign_launch(b, c->ecdsas.table_p256.as<uint32_t>(), c->ecdsas.scratch.buf.as<uint32_t>(),
                                         d_sig, s));
  } else {
    CBFT_HIP(cbft_ecdsa_sign_launch(b, c->ecdsas.table.as<uint32_t>(), c->ecdsas.scratch.buf.as<uint32_t>(), d_sig, s));
  }
  CBFT_HIP(c->ecdsas.timer.end(c->profiling, s));
  CBFT_HIP(c->ecdsas.scratch.commit(s));
  return CBFT_OK;
}

void cbft_ecdsa_sign_release(cbft_ctx* c) {
  (void)hipSetDevice(c->device);
  c->ecdsas.scratch.drain_and_zero(c->stream);  // synchronises the device: device-path batches run on caller streams
  for (auto& kv : c->ecdsa_signer_tables) cbft_clear_release(kv.second.rec, c->stream);
  (void)hipStreamSynchronize(c->stream);
  c->ecdsa_signer_tables.clear();
  for (DevBuf* b : {&c->ecdsas.table, &c->ecdsas.table_p256, &c->ecdsas.in, &c->ecdsas.out}) b->release();
  c->ecdsas.scratch.release();
  c->ecdsas.timer.release();
}

static EcdsaSignerTable* ecdsas_find(cbft_ctx* c, uint32_t id) {
  auto it = c->ecdsa_signer_tables.find(id);
  return it == c->ecdsa_signer_tables.end() ? nullptr : &it->second;
}

extern "C" {

int cbft_ecdsa_load_signers(cbft_ctx* c, const uint8_t* priv, uint32_t nkeys, uint32_t* out_id) {
  return cbft_ecdsa_load_signers_curve(c, CBFT_CURVE_SECP256K1, priv, nkeys, out_id);
}

int cbft_ecdsa_load_signers_curve(cbft_ctx* c, int curve, const uint8_t* priv, uint32_t nkeys, uint32_t* out_id) {
  c = cbft_dev0(c);
  if (!c) return CBFT_EINVAL;
  if (curve != CBFT_CURVE_SECP256K1 && curve != CBFT_CURVE_P256) return CBFT_EINVAL;
  if (nkeys > CBFT_ECDSA_MAX_KEYS) return CBFT_E2BIG;
  if (!priv || !out_id || nkeys == 0) return CBFT_EINVAL;
  const bool p256 = curve == CBFT_CURVE_P256;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  DevBuf& comb = p256 ? c->ecdsas.table_p256 : c->ecdsas.table;
  if (!comb.p) {
    CBFT_HIP(comb.reserve((size_t)ECDSAS_TABLE_WORDS * sizeof(uint32_t)));
    hipError_t e = p256 ? cbft_ecdsa_p256_sign_build_table(comb.as<uint32_t>(), c->stream)
                        : cbft_ecdsa_sign_build_table(comb.as<uint32_t>(), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
      comb.release();
      return cbft_fail(e, "ecdsa sign comb table", __FILE__, __LINE__);
    }
  }
  EcdsaSignerTable st;
  st.nkeys = nkeys;
  st.curve = curve;
  const size_t kbytes = (size_t)nkeys * ECDSAS_PRIV_BYTES;
  CBFT_HIP(st.rec.reserve((size_t)nkeys * ECDSAS_WORDS * sizeof(uint32_t)));
  HostBuf hs;
  DevBuf ds;
  hipError_t e = hs.reserve(kbytes);
  if (e == hipSuccess) e = ds.reserve(kbytes);
  if (e == hipSuccess) {
    std::memcpy(hs.p, priv, kbytes);
    e = hipMemcpyAsync(ds.p, hs.p, kbytes, hipMemcpyHostToDevice, c->stream);
  }
  if (e == hipSuccess)
    e = p256 ? cbft_ecdsa_p256_sign_launch_keys(ds.as<uint8_t>(), nkeys, comb.as<uint32_t>(), st.rec.as<uint32_t>(),
                                                c->stream)
             : cbft_ecdsa_sign_launch_keys(ds.as<uint8_t>(), nkeys, comb.as<uint32_t>(), st.rec.as<uint32_t>(),
                                           c->stream);
  const hipError_t e2 = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = e2;
  if (hs.p) cbft_wipe(hs.p, hs.cap);  // the keys are on the device (or the load failed): none stay here
  hs.release();
  cbft_clear_release(ds, c->stream);  // whether or not the records were built, the raw keys are cleared before the free
  if (e != hipSuccess) {
    cbft_clear_release(st.rec, c->stream);
    return cbft_fail(e, "ecdsa signer records", __FILE__, __LINE__);
  }
  const uint32_t id = c->next_ecdsa_signer_id++;
  c->ecdsa_signer_tables.emplace(id, std::move(st));
  *out_id = id;
  return CBFT_OK;
}

int cbft_ecdsa_signer_status(cbft_ctx* c, uint32_t id, uint8_t* out_ok) {
  c = cbft_dev0(c);
  if (!c || !out_ok) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  EcdsaSignerTable* st = ecdsas_find(c, id);
  if (!st) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  std::vector<uint32_t> ok(st->nkeys);
  // only the validity word of each record crosses to the host
  CBFT_HIP(hipMemcpy2D(ok.data(), sizeof(uint32_t), st->rec.as<uint32_t>() + ECDSAS_OK, ECDSAS_WORDS * sizeof(uint32_t),
                       sizeof(uint32_t), st->nkeys, hipMemcpyDeviceToHost));
  for (uint32_t k = 0; k < st->nkeys; k++) out_ok[k] = ok[k] ? 1 : 0;
  return CBFT_OK;
}

int cbft_ecdsa_signer_public_keys(cbft_ctx* c, uint32_t id, uint8_t* out_pub) {
  c = cbft_dev0(c);
  if (!c || !out_pub) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  EcdsaSignerTable* st = ecdsas_find(c, id);
  if (!st) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  // only the Q part of each record crosses to the host (limbs there, big-endian bytes here)
  std::vector<uint32_t> q((size_t)st->nkeys * 16);
  CBFT_HIP(hipMemcpy2D(q.data(), 64, st->rec.as<uint32_t>() + 8, ECDSAS_WORDS * sizeof(uint32_t), 64, st->nkeys,
                       hipMemcpyDeviceToHost));
  for (uint32_t k = 0; k < st->nkeys; k++) {
    k1_to_be(out_pub + (size_t)k * 64, q.data() + (size_t)k * 16);
    k1_to_be(out_pub + (size_t)k * 64 + 32, q.data() + (size_t)k * 16 + 8);
  }
  return CBFT_OK;
}

int cbft_ecdsa_unload_signers(cbft_ctx* c, uint32_t id) {
  c = cbft_dev0(c);
  if (!c) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->ecdsa_signer_tables.find(id);
  if (it == c->ecdsa_signer_tables.end()) return CBFT_EINVAL;
  (void)hipSetDevice(c->device);
  // synchronises the device first: in-flight device-path batches on caller streams read the table
  c->ecdsas.scratch.drain_and_zero(c->stream);
  cbft_clear_release(it->second.rec, c->stream);
  c->ecdsa_signer_tables.erase(it);
  return CBFT_OK;
}

int cbft_ecdsa_sign_batch(cbft_ctx* c, uint32_t id, const uint32_t* signer_idx, const uint8_t* msg_blob,
                          const uint64_t* msg_off, const uint32_t* msg_len, size_t n, uint8_t* out_sig) {
  c = cbft_dev0(c);
  if (!c) return CBFT_EINVAL;
  if (n > CBFT_ECDSA_MAX_BATCH) return CBFT_E2BIG;
  if (n && (!msg_off || !msg_len || !out_sig)) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  EcdsaSignerTable* st = ecdsas_find(c, id);
  if (!st) return CBFT_EINVAL;
  if (n == 0) return CBFT_OK;
  for (size_t i = 0; i < n; i++)
    if (signer_idx && signer_idx[i] >= st->nkeys) return CBFT_EINVAL;
  c->host_off.resize(n);
  const CbftSpan span = cbft_msg_span(msg_off, msg_len, n, CBFT_MAX_MSG_LEN, msg_blob != nullptr, c->host_off.data());
  if (span.err) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  const CbftPackedArray idx{signer_idx, n * 4};
  CbftPackedLayout L;
  CBFT_HIP(cbft_upload_packed(c->ecdsas.in, c->stream, c->host_off.data(), msg_len, n, &idx, 1, msg_blob, span, &L));
  CBFT_HIP(c->ecdsas.out.reserve(n * 64));
  const uint8_t* d = c->ecdsas.in.as<uint8_t>();
  const int rc = ecdsas_launch_locked(c, *st, signer_idx ? reinterpret_cast<const uint32_t*>(d + L.mid[0]) : nullptr,
                                      d + L.blob, reinterpret_cast<const uint64_t*>(d + L.off),
                                      reinterpret_cast<const uint32_t*>(d + L.len), 0, n, c->ecdsas.out.as<uint8_t>(),
                                      c->stream);
  if (rc) return rc;
  CBFT_HIP(hipMemcpyAsync(out_sig, c->ecdsas.out.p, n * 64, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  return CBFT_OK;
}

int cbft_ecdsa_sign_fixed_device(cbft_ctx* c, uint32_t id, const uint32_t* d_signer_idx, const uint8_t* d_msg,
                                 uint32_t msg_len, size_t n, uint8_t* d_sig, void* stream) {
  if (c && !c->kids.empty()) return CBFT_EINVAL;  // device pointers belong to one GPU: use its own context
  if (!c) return CBFT_EINVAL;
  if (n > CBFT_ECDSA_MAX_BATCH) return CBFT_E2BIG;
  if (n && (!d_sig || (msg_len && !d_msg))) return CBFT_EINVAL;
  if (msg_len > CBFT_MAX_MSG_LEN) return CBFT_EINVAL;
  if (reinterpret_cast<uintptr_t>(d_sig) & 3) return CBFT_EINVAL;  // signatures are written as words
  std::lock_guard<std::mutex> g(c->mu);
  EcdsaSignerTable* st = ecdsas_find(c, id);
  if (!st) return CBFT_EINVAL;
  if (n == 0) return CBFT_OK;
  CBFT_HIP(hipSetDevice(c->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  return ecdsas_launch_locked(c, *st, d_signer_idx, d_msg, nullptr, nullptr, msg_len, n, d_sig, s);
}

int cbft_ecdsa_sign_kernel_ms(cbft_ctx* c, float* out_ms) {
  c = cbft_dev0(c);
  if (!c || !out_ms) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->ecdsas.timer.valid) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(c->ecdsas.timer.elapsed(out_ms));
  return CBFT_OK;
}

}  // extern "C"
