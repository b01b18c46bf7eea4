// libcbft_hipcrypto, RSA signing half of the C ABI (include/cbft_hipcrypto.h).
//
// The batch form of concord::util::crypto::RSASigner::sign, the signer SigManager holds for an RSA
// replica key: a signer table is loaded once (CRT records built and self-tested on the GPU) and
// every sign is a batch on the GPU (rsa_sign.hip), followed by the public check s^e mod n == EM
// with the verify kernel (rsa_verify.hip) and a gate that withholds what did not pass.
//
// Multi-GPU contexts: signer tables live on the lowest device (cbft_dev0) and the host-array calls
// run there, like the Ed25519 signing calls; the _device entry needs a single-GPU context.
//
// Secrets: the keys pass through pinned staging that is zeroed once they are on the device, the
// device copy of the raw key bytes is cleared after the records are built, the window tables are
// zeroed by the signing kernel before it ends and again with the records when a table is unloaded
// and at close.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "cbft_internal.h"

static_assert(CBFT_RSA_PRIVATE_KEY_BYTES == RSAS_PRIV_BYTES && CBFT_RSA_SIGNATURE_BYTES == 256, "sizes");

static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// sign, check (verify kernel on the fresh signatures), gate.  use_status = 0 only for the
// load-time self-test, whose verdict words (at the returned pointer) become the status.
static int rsa_sign_launch_locked(cbft_ctx* c, RsaSignerTable& st, const uint32_t* d_idx, const uint8_t* d_msg,
                                  const uint64_t* d_off, const uint32_t* d_len, uint32_t fixed_len, size_t n,
                                  uint8_t* d_sig, int use_status, bool want_failed, uint64_t** out_verdicts,
                                  uint32_t** out_failed, hipStream_t s) {
  const size_t o_idx = 0, o_off = align16(n * 4), o_len = o_off + n * 8, o_verd = align16(o_len + n * 4),
               o_fail = o_verd + ((n + 63) / 64) * 8;
  CBFT_HIP(c->rsas.aux.reserve(o_fail + 16));
  CBFT_HIP(c->rsas.vscratch.reserve(cbft_rsa_scratch_words(n) * sizeof(uint32_t)));
  CBFT_HIP(c->rsas.scratch.acquire(cbft_rsa_sign_scratch_words(n) * sizeof(uint32_t), s));  // orders all three
  uint8_t* aux = c->rsas.aux.as<uint8_t>();
  uint32_t* v_idx = reinterpret_cast<uint32_t*>(aux + o_idx);
  uint64_t* v_off = reinterpret_cast<uint64_t*>(aux + o_off);
  uint32_t* v_len = reinterpret_cast<uint32_t*>(aux + o_len);
  uint64_t* verd = reinterpret_cast<uint64_t*>(aux + o_verd);
  uint32_t* failed = reinterpret_cast<uint32_t*>(aux + o_fail);
  RsaSignBatch b{n, st.rec.as<uint32_t>(), st.nkeys, d_idx, d_msg, d_off, d_len, fixed_len};
  if (want_failed) CBFT_HIP(hipMemsetAsync(failed, 0, 4, s));
  CBFT_HIP(cbft_rsa_sign_launch(b, c->rsas.scratch.buf.as<uint32_t>(), d_sig, s));
  CBFT_HIP(cbft_rsa_sign_launch_prep(b, v_idx, v_off, v_len, s));
  RsaBatch vb{n, st.vrec.as<uint32_t>(), st.nkeys, v_idx, d_sig, d_msg, v_off, v_len};
  CBFT_HIP(cbft_rsa_launch_verify(vb, c->rsas.vscratch.as<uint32_t>(), verd, s));
  CBFT_HIP(cbft_rsa_sign_launch_gate(b, verd, use_status, d_sig, want_failed ? failed : nullptr, s));
  CBFT_HIP(c->rsas.scratch.commit(s));
  if (out_verdicts) *out_verdicts = verd;
  if (out_failed) *out_failed = failed;
  return CBFT_OK;
}

static void clear_table(cbft_ctx* c, RsaSignerTable& st) {
  cbft_clear_release(st.rec, c->stream);
  st.vrec.release();
}

void cbft_rsa_sign_release(cbft_ctx* c) {
  (void)hipSetDevice(c->device);
  c->rsas.scratch.drain_and_zero(c->stream);
  for (auto& kv : c->rsa_signer_tables) clear_table(c, kv.second);
  (void)hipStreamSynchronize(c->stream);
  c->rsa_signer_tables.clear();
  for (DevBuf* b : {&c->rsas.aux, &c->rsas.vscratch, &c->rsas.in, &c->rsas.out}) b->release();
  c->rsas.scratch.release();
}

extern "C" {

int cbft_rsa_load_signers(cbft_ctx* c, const uint8_t* priv, const uint32_t* exponents, uint32_t nkeys,
                          uint32_t* out_id) {
  c = cbft_dev0(c);
  if (!c || !priv || !exponents || !out_id || nkeys == 0) return CBFT_EINVAL;
  if (nkeys > (1u << 16)) return CBFT_E2BIG;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  RsaSignerTable st;
  st.nkeys = nkeys;
  const size_t pbytes = (size_t)nkeys * RSAS_PRIV_BYTES;
  CBFT_HIP(st.rec.reserve((size_t)nkeys * RSAS_WORDS * sizeof(uint32_t)));
  CBFT_HIP(st.vrec.reserve((size_t)nkeys * RSA_KEY_WORDS * sizeof(uint32_t)));
  HostBuf hs;
  DevBuf dp, dex, dmod, didx, dmsg, dsig;
  hipError_t e = hs.reserve(pbytes);
  if (e == hipSuccess) e = dp.reserve(pbytes);
  if (e == hipSuccess) e = dex.reserve((size_t)nkeys * 4);
  if (e == hipSuccess) e = dmod.reserve((size_t)nkeys * RSA_MOD_BYTES);
  if (e == hipSuccess) e = didx.reserve((size_t)nkeys * 4);
  if (e == hipSuccess) e = dmsg.reserve((size_t)nkeys * 32);
  if (e == hipSuccess) e = dsig.reserve((size_t)nkeys * 256);
  std::vector<uint32_t> iota(nkeys);
  for (uint32_t k = 0; k < nkeys; k++) iota[k] = k;
  if (e == hipSuccess) {
    std::memcpy(hs.p, priv, pbytes);
    e = hipMemcpyAsync(dp.p, hs.p, pbytes, hipMemcpyHostToDevice, c->stream);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(dex.p, exponents, (size_t)nkeys * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(didx.p, iota.data(), (size_t)nkeys * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(dmsg.p, 0x5a, (size_t)nkeys * 32, c->stream);  // the self-test message
  if (e == hipSuccess)
    e = cbft_rsa_sign_launch_keys(dp.as<uint8_t>(), dex.as<uint32_t>(), nkeys, st.rec.as<uint32_t>(),
                                  dmod.as<uint8_t>(), c->stream);
  if (e == hipSuccess && dp.p) e = hipMemsetAsync(dp.p, 0, dp.cap, c->stream);
  if (e == hipSuccess)
    e = cbft_rsa_launch_keys(dmod.as<uint8_t>(), dex.as<uint32_t>(), nkeys, st.vrec.as<uint32_t>(), c->stream);
  int rc = CBFT_OK;
  if (e == hipSuccess) {
    // self-test: one signature per key, checked with the public operation; the verdicts and the
    // structural checks make the status words
    uint64_t* verd = nullptr;
    rc = rsa_sign_launch_locked(c, st, didx.as<uint32_t>(), dmsg.as<uint8_t>(), nullptr, nullptr, 32, nkeys,
                                dsig.as<uint8_t>(), 0, false, &verd, nullptr, c->stream);
    if (rc == CBFT_OK) e = cbft_rsa_sign_launch_status(st.rec.as<uint32_t>(), nkeys, verd, c->stream);
  }
  const hipError_t e2 = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = e2;
  if (hs.p) cbft_wipe(hs.p, hs.cap);  // the keys are on the device (or the load failed): none stay here
  hs.release();
  for (DevBuf* b : {&dp, &dex, &dmod, &didx, &dmsg, &dsig}) b->release();
  if (e != hipSuccess || rc != CBFT_OK) {
    clear_table(c, st);
    return rc != CBFT_OK ? rc : cbft_fail(e, "rsa signer records", __FILE__, __LINE__);
  }
  const uint32_t id = c->next_rsa_signer_id++;
  c->rsa_signer_tables.emplace(id, std::move(st));
  *out_id = id;
  return CBFT_OK;
}

int cbft_rsa_signer_status(cbft_ctx* c, uint32_t id, uint8_t* out_ok) {
  c = cbft_dev0(c);
  if (!c || !out_ok) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->rsa_signer_tables.find(id);
  if (it == c->rsa_signer_tables.end()) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  // only the status word of each record crosses to the host
  std::vector<uint32_t> st(it->second.nkeys);
  CBFT_HIP(hipMemcpy2D(st.data(), 4, it->second.rec.as<uint32_t>() + RSAS_STATUS, RSAS_WORDS * sizeof(uint32_t), 4,
                       it->second.nkeys, hipMemcpyDeviceToHost));
  for (uint32_t k = 0; k < it->second.nkeys; k++) out_ok[k] = st[k] == 1u ? 1 : 0;
  return CBFT_OK;
}

int cbft_rsa_signer_moduli(cbft_ctx* c, uint32_t id, uint8_t* out_n) {
  c = cbft_dev0(c);
  if (!c || !out_n) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->rsa_signer_tables.find(id);
  if (it == c->rsa_signer_tables.end()) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  // n as the verify record holds it: 64 little-endian words
  std::vector<uint32_t> w((size_t)it->second.nkeys * RSA_LIMBS);
  CBFT_HIP(hipMemcpy2D(w.data(), RSA_LIMBS * 4, it->second.vrec.as<uint32_t>() + RSA_KEY_N,
                       RSA_KEY_WORDS * sizeof(uint32_t), RSA_LIMBS * 4, it->second.nkeys, hipMemcpyDeviceToHost));
  for (uint32_t k = 0; k < it->second.nkeys; k++)
    for (int i = 0; i < RSA_LIMBS; i++) {
      const uint32_t v = w[(size_t)k * RSA_LIMBS + (RSA_LIMBS - 1 - i)];
      uint8_t* o = out_n + (size_t)k * RSA_MOD_BYTES + 4 * i;
      o[0] = (uint8_t)(v >> 24), o[1] = (uint8_t)(v >> 16), o[2] = (uint8_t)(v >> 8), o[3] = (uint8_t)v;
    }
  return CBFT_OK;
}

int cbft_rsa_unload_signers(cbft_ctx* c, uint32_t id) {
  c = cbft_dev0(c);
  if (!c) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->rsa_signer_tables.find(id);
  if (it == c->rsa_signer_tables.end()) return CBFT_EINVAL;
  (void)hipSetDevice(c->device);
  // synchronises the device first: in-flight device-path batches read the table
  c->rsas.scratch.drain_and_zero(c->stream);
  clear_table(c, it->second);
  c->rsa_signer_tables.erase(it);
  return CBFT_OK;
}

int cbft_rsa_sign_batch(cbft_ctx* c, uint32_t id, const uint32_t* signer_idx, const uint8_t* msg_blob,
                        const uint64_t* msg_off, const uint32_t* msg_len, size_t n, uint8_t* out_sig,
                        uint32_t* out_failed) {
  c = cbft_dev0(c);
  if (!c || (n && (!msg_off || !msg_len || !out_sig))) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->rsa_signer_tables.find(id);
  if (it == c->rsa_signer_tables.end()) return CBFT_EINVAL;
  if (out_failed && n == 0) *out_failed = 0;
  if (n == 0) return CBFT_OK;
  for (size_t i = 0; i < n; i++)
    if (signer_idx && signer_idx[i] >= it->second.nkeys) return CBFT_EINVAL;
  c->host_off.resize(n);
  const CbftSpan span = cbft_msg_span(msg_off, msg_len, n, CBFT_MAX_MSG_LEN, msg_blob != nullptr, c->host_off.data());
  if (span.err) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  const CbftPackedArray idx{signer_idx, n * 4};
  CbftPackedLayout L;
  CBFT_HIP(cbft_upload_packed(c->rsas.in, c->stream, c->host_off.data(), msg_len, n, &idx, 1, msg_blob, span, &L));
  CBFT_HIP(c->rsas.out.reserve(n * 256));
  const uint8_t* d = c->rsas.in.as<uint8_t>();
  uint32_t* d_failed = nullptr;
  const int rc = rsa_sign_launch_locked(
      c, it->second, signer_idx ? reinterpret_cast<const uint32_t*>(d + L.mid[0]) : nullptr, d + L.blob,
      reinterpret_cast<const uint64_t*>(d + L.off), reinterpret_cast<const uint32_t*>(d + L.len), 0, n,
      c->rsas.out.as<uint8_t>(), 1, true, nullptr, &d_failed, c->stream);
  if (rc) return rc;
  uint32_t failed = 0;
  CBFT_HIP(hipMemcpyAsync(&failed, d_failed, 4, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipMemcpyAsync(out_sig, c->rsas.out.p, n * 256, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  if (out_failed) *out_failed = failed;
  return CBFT_OK;
}

int cbft_rsa_sign_fixed_device(cbft_ctx* c, uint32_t id, const uint32_t* d_signer_idx, const uint8_t* d_msg,
                               uint32_t msg_len, size_t n, uint8_t* d_sig, void* stream) {
  if (c && !c->kids.empty()) return CBFT_EINVAL;  // device pointers belong to one GPU: use its own context
  if (!c || (n && (!d_sig || (msg_len && !d_msg)))) return CBFT_EINVAL;
  if (msg_len > CBFT_MAX_MSG_LEN) return CBFT_EINVAL;
  if (reinterpret_cast<uintptr_t>(d_sig) & 3) return CBFT_EINVAL;  // signatures are written as words
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->rsa_signer_tables.find(id);
  if (it == c->rsa_signer_tables.end()) return CBFT_EINVAL;
  if (n == 0) return CBFT_OK;
  CBFT_HIP(hipSetDevice(c->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  return rsa_sign_launch_locked(c, it->second, d_signer_idx, d_msg, nullptr, nullptr, msg_len, n, d_sig, 1, false,
                                nullptr, nullptr, s);
}

}  // extern "C"
