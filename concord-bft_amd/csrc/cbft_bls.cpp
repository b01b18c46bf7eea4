// libcbft_hipcrypto, BLS BN-P254 half of the C ABI (include/cbft_hipcrypto.h).
//
// Mirrors threshsign's verifier/accumulator work: key sets are
// decoded and their G2 Miller-loop lines precomputed once (cbft_bls_load_keys, like
// BlsThresholdVerifier's constructor holding the decoded keys); every per-certificate call
// runs on the GPU: hash-to-G1, share decompression + pairing checks, Lagrange coefficients,
// the multi-scalar multiplication, the combined-signature check.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>
#include <thread>

#include "bls_kernels.h"
#include "cbft_internal.h"

static_assert(CBFT_BLS_G1_PARTIAL_BYTES == BLS_JAC_WORDS * 4, "G1 partial layout");
static_assert(CBFT_BLS_G2_PARTIAL_BYTES == BLS_G2_PART_WORDS * 4, "G2 partial layout");

#define BLS_MAX_SHARES 2048  // IThresholdVerifier::maxSize_ (IThresholdVerifier.h:36)

static int bls_gen_lines(cbft_ctx* c) {
  if (c->bls_gen_lines.p) return CBFT_OK;
  CBFT_HIP(c->bls_gen_lines.reserve(cbft_bls_lines_words_per_key() * 4));
  CBFT_HIP(cbft_bls_launch_gen_lines(c->bls_gen_lines.as<uint32_t>(), c->stream));
  return CBFT_OK;
}

static int bls_upload_msg(cbft_ctx* c, const uint8_t* msg, uint32_t len) {
  CBFT_HIP(c->bls_msg.reserve(len + 1));
  CBFT_HIP(c->bls_H.reserve(19 * 4));
  if (len) CBFT_HIP(hipMemcpyAsync(c->bls_msg.p, msg, len, hipMemcpyHostToDevice, c->stream));
  return CBFT_OK;
}

static int bls_upload_msg_hash(cbft_ctx* c, const uint8_t* msg, uint32_t len) {
  int rc = bls_upload_msg(c, msg, len);
  if (rc) return rc;
  CBFT_HIP(cbft_bls_launch_hash(c->bls_msg.as<uint8_t>(), len, c->bls_H.as<uint32_t>(), c->stream));
  return CBFT_OK;
}

static BlsKeySet* find_set(cbft_ctx* c, uint32_t id) {
  auto it = c->bls_sets.find(id);
  return it == c->bls_sets.end() ? nullptr : &it->second;
}

extern "C" {

int cbft_bls_load_keys(cbft_ctx* c, const uint8_t* pk65, const uint8_t* vks65, uint32_t n, uint32_t* out_id) {
  if (c && !c->kids.empty()) {  // multi-GPU: the key set on every device, the ids kept in step
    if (!pk65 || !out_id || (n && !vks65) || n > BLS_MAX_SHARES) return CBFT_EINVAL;
    std::vector<uint32_t> ids(c->kids.size(), 0);
    const int rc = for_each_kid(c, [&](size_t g) { return cbft_bls_load_keys(c->kids[g], pk65, vks65, n, &ids[g]); });
    if (rc) return rc;
    for (uint32_t id : ids)
      if (id != ids[0]) return CBFT_EIO;
    *out_id = ids[0];
    return CBFT_OK;
  }
  if (!c || !pk65 || !out_id || (n && !vks65) || n > BLS_MAX_SHARES) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  int rc = bls_gen_lines(c);
  if (rc) return rc;
  BlsKeySet ks;
  ks.n = n;
  const size_t nk = (size_t)n + 1;  // slot 0 = group PK
  CBFT_HIP(ks.keys65.reserve(nk * 65));
  CBFT_HIP(ks.lines.reserve(nk * cbft_bls_lines_words_per_key() * 4));
  CBFT_HIP(ks.ok.reserve(nk));
  CBFT_HIP(ks.aff.reserve(nk * BLS_G2A_WORDS * 4));
  CBFT_HIP(hipMemcpyAsync(ks.keys65.p, pk65, 65, hipMemcpyHostToDevice, c->stream));
  if (n)
    CBFT_HIP(hipMemcpyAsync(ks.keys65.as<uint8_t>() + 65, vks65, (size_t)n * 65, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(cbft_bls_launch_keys(ks.keys65.as<uint8_t>(), (uint32_t)nk, ks.lines.as<uint32_t>(), ks.ok.as<uint8_t>(),
                                ks.aff.as<uint32_t>(), c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  uint32_t id = c->next_bls_id++;
  c->bls_sets.emplace(id, std::move(ks));
  *out_id = id;
  return CBFT_OK;
}

int cbft_bls_unload_keys(cbft_ctx* c, uint32_t id) {
  if (c && !c->kids.empty()) {
    int rc = CBFT_OK;
    for (cbft_ctx* k : c->kids) {
      const int r = cbft_bls_unload_keys(k, id);
      if (r && !rc) rc = r;
    }
    return rc;
  }
  if (!c) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  BlsKeySet* ks = find_set(c, id);
  if (!ks) return CBFT_EINVAL;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  ks->keys65.release();
  ks->lines.release();
  ks->ok.release();
  ks->aff.release();
  c->bls_sets.erase(id);
  return CBFT_OK;
}

int cbft_bls_key_status(cbft_ctx* c, uint32_t id, uint8_t* out_ok) {
  c = cbft_dev0(c);
  if (!c || !out_ok) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  BlsKeySet* ks = find_set(c, id);
  if (!ks) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(hipMemcpy(out_ok, ks->ok.p, ks->n + 1, hipMemcpyDeviceToHost));
  return CBFT_OK;
}

int cbft_bls_hash_to_g1(cbft_ctx* c, const uint8_t* msg, uint32_t len, uint8_t* out33) {
  c = cbft_dev0(c);
  if (!c || !out33 || (len && !msg)) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  int rc = bls_upload_msg_hash(c, msg, len);
  if (rc) return rc;
  // compress through the MSM finish kernel path: reuse combine with one unit share is
  // overkill; instead read H back and compress on the device via a 1-share multisig combine
  CBFT_HIP(c->bls_use.reserve(1));
  CBFT_HIP(c->bls_partial.reserve(27 * 4));
  CBFT_HIP(c->bls_out.reserve(33));
  uint8_t one = 1;
  CBFT_HIP(hipMemcpyAsync(c->bls_use.p, &one, 1, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(cbft_bls_launch_combine(c->bls_H.as<uint32_t>(), nullptr, c->bls_use.as<uint8_t>(), 1, 0, 1, 1, nullptr,
                                   nullptr, c->bls_partial.as<uint32_t>(), c->bls_out.as<uint8_t>(), nullptr, nullptr,
                                   c->stream));
  CBFT_HIP(hipMemcpyAsync(out33, c->bls_out.p, 33, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  return CBFT_OK;
}

// Stage k shares on the device and decode them, one lane per share (ids, affine points, valid =
// decodable && id in range), hashing the uploaded message to bls_H in the same launch when
// `hash` (the share roots run beside the hash instead of after it).
static int bls_prep(cbft_ctx* c, BlsKeySet* ks, const uint8_t* shares37, uint32_t k, bool hash, uint32_t len) {
  CBFT_HIP(c->bls_shares.reserve((size_t)(k ? k : 1) * 37));
  CBFT_HIP(c->bls_valid.reserve(k ? k : 1));
  CBFT_HIP(c->bls_sig.reserve((size_t)(k ? k : 1) * BLS_SIG_WORDS * 4));
  CBFT_HIP(c->bls_ids.reserve((size_t)(k ? k : 1) * 4));
  if (k) CBFT_HIP(hipMemcpyAsync(c->bls_shares.p, shares37, (size_t)k * 37, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(cbft_bls_launch_prep(c->bls_msg.as<uint8_t>(), len, hash ? c->bls_H.as<uint32_t>() : nullptr,
                                c->bls_shares.as<uint8_t>(), k, ks ? ks->n : BLS_MAX_SHARES,
                                c->bls_valid.as<uint8_t>(), c->bls_sig.as<uint32_t>(), c->bls_ids.as<uint32_t>(),
                                c->stream));
  return CBFT_OK;
}

// Verify the k shares bls_prep decoded against H (bls_H): verdicts into bls_valid.
static int bls_verify_parsed(cbft_ctx* c, BlsKeySet* ks, uint32_t k) {
  CBFT_HIP(cbft_bls_launch_share_verify(
      c->bls_shares.as<uint8_t>(), k, ks->n, c->bls_H.as<uint32_t>(),
      ks->lines.as<uint32_t>() + cbft_bls_lines_words_per_key(), ks->ok.as<uint8_t>() + 1,
      c->bls_gen_lines.as<uint32_t>(), 1, 1, c->bls_valid.as<uint8_t>(), c->bls_sig.as<uint32_t>(),
      c->bls_ids.as<uint32_t>(), c->stream));
  return CBFT_OK;
}

int cbft_bls_verify_shares(cbft_ctx* c, uint32_t id, const uint8_t* msg, uint32_t len, const uint8_t* shares37,
                           uint32_t k, uint8_t* valid_bitmap) {
  if (c && !c->kids.empty()) {
    // multi-GPU: contiguous share slices, one per device, verified
    // concurrently against the device's copy of the key set; the slice bitmaps are merged
    if ((k && (!shares37 || !valid_bitmap)) || (len && !msg) || k > BLS_MAX_SHARES) return CBFT_EINVAL;
    if (!k) return CBFT_OK;
    const size_t G = c->kids.size(), per = (k + G - 1) / G;
    std::vector<std::vector<uint8_t>> part(G);
    const int rc = for_each_kid(c, [&](size_t g) {
      const size_t lo = std::min<size_t>(k, g * per), hi = std::min<size_t>(k, lo + per);
      part[g].assign((hi - lo + 7) / 8 + 1, 0);
      if (hi == lo) return (int)CBFT_OK;
      return cbft_bls_verify_shares(c->kids[g], id, msg, len, shares37 + 37 * lo, (uint32_t)(hi - lo), part[g].data());
    });
    if (rc) return rc;
    std::memset(valid_bitmap, 0, (k + 7) / 8);
    for (size_t g = 0; g < G; g++) {
      const size_t lo = std::min<size_t>(k, g * per), hi = std::min<size_t>(k, lo + per);
      for (size_t j = lo; j < hi; j++)
        if ((part[g][(j - lo) >> 3] >> ((j - lo) & 7)) & 1) valid_bitmap[j >> 3] |= (uint8_t)(1u << (j & 7));
    }
    return CBFT_OK;
  }
  if (!c || (k && (!shares37 || !valid_bitmap)) || (len && !msg) || k > BLS_MAX_SHARES) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  BlsKeySet* ks = find_set(c, id);
  if (!ks) return CBFT_EINVAL;
  if (!k) return CBFT_OK;
  CBFT_HIP(hipSetDevice(c->device));
  int rc = bls_gen_lines(c);
  if (!rc) rc = bls_upload_msg(c, msg, len);
  if (!rc) rc = bls_prep(c, ks, shares37, k, true, len);
  if (!rc) rc = bls_verify_parsed(c, ks, k);
  if (rc) return rc;
  std::vector<uint8_t> v(k);
  CBFT_HIP(hipMemcpyAsync(v.data(), c->bls_valid.p, k, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  std::memset(valid_bitmap, 0, (k + 7) / 8);
  for (uint32_t j = 0; j < k; j++)
    if (v[j]) valid_bitmap[j >> 3] |= (uint8_t)(1u << (j & 7));
  return CBFT_OK;
}

// Parse k shares (distinct ids, all decodable) onto the device and launch lambda + the MSM over
// [lo, hi): into out33 (compressed), or into out_part (one Jacobian partial) when non-null.
static int bls_combine_range(cbft_ctx* c, const uint8_t* shares37, uint32_t k, uint32_t lo, uint32_t hi, int multisig,
                             uint8_t* out33, uint8_t* out_part) {
  // distinct ids (the accumulators never hold two shares of one signer)
  std::vector<uint8_t> seen(1u << 16, 0);
  for (uint32_t j = 0; j < k; j++) {
    const uint8_t* s = shares37 + 37 * (size_t)j;
    const uint32_t sid = ((uint32_t)s[0] << 24) | ((uint32_t)s[1] << 16) | ((uint32_t)s[2] << 8) | s[3];
    if (sid == 0 || sid > BLS_MAX_SHARES || seen[sid]) return CBFT_EINVAL;
    seen[sid] = 1;
  }
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  int rc = bls_prep(c, nullptr, shares37, k, false, 0);
  if (rc) return rc;
  CBFT_HIP(c->bls_lambda.reserve((size_t)k * 8 * 4));
  CBFT_HIP(c->bls_partial.reserve((size_t)(2 * k + 16) * BLS_JAC_WORDS * 4));  // row MSM levels
  CBFT_HIP(c->bls_out.reserve(BLS_JAC_WORDS * 4));
  // every share decoded? (the parse kernel wrote valid = decodable && id in range).  Checked after
  // the combine, in the same synchronisation: the combine only reads the shares valid marks, and its
  // result is discarded when any share failed to decode (one host round trip instead of two).
  std::vector<uint8_t> v(k);
  if (!multisig && !c->bls_inv.p) {  // inverses of 1..2048 mod r, once per context
    CBFT_HIP(c->bls_inv.reserve((size_t)BLS_INV_TABLE * 9 * 4));
    CBFT_HIP(cbft_bls_launch_inv_table(c->bls_inv.as<uint32_t>(), c->stream));
  }
  CBFT_HIP(cbft_bls_launch_combine(c->bls_sig.as<uint32_t>(), c->bls_ids.as<uint32_t>(), c->bls_valid.as<uint8_t>(),
                                   k, lo, hi, multisig, c->bls_inv.as<uint32_t>(), c->bls_lambda.as<uint32_t>(),
                                   c->bls_partial.as<uint32_t>(),
                                   c->bls_out.as<uint8_t>(), nullptr,
                                   out_part ? c->bls_out.as<uint32_t>() : nullptr, c->stream));
  std::vector<uint8_t> res(out_part ? CBFT_BLS_G1_PARTIAL_BYTES : 33);
  CBFT_HIP(hipMemcpyAsync(res.data(), c->bls_out.p, res.size(), hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipMemcpyAsync(v.data(), c->bls_valid.p, k, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  for (uint32_t j = 0; j < k; j++)
    if (!v[j]) return CBFT_EINVAL;  // outputs untouched
  std::memcpy(out_part ? out_part : out33, res.data(), res.size());
  return CBFT_OK;
}

int cbft_bls_combine(cbft_ctx* c, const uint8_t* shares37, uint32_t k, int multisig, uint8_t* out33) {
  c = cbft_dev0(c);
  if (!c || !out33 || !k || !shares37 || k > BLS_MAX_SHARES) return CBFT_EINVAL;
  return bls_combine_range(c, shares37, k, 0, k, multisig, out33, nullptr);
}

int cbft_bls_combine_partial(cbft_ctx* c, const uint8_t* shares37, uint32_t k, uint32_t lo, uint32_t hi, int multisig,
                             uint8_t* out_partial) {
  c = cbft_dev0(c);
  if (!c || !out_partial || !k || !shares37 || k > BLS_MAX_SHARES || lo > hi || hi > k) return CBFT_EINVAL;
  return bls_combine_range(c, shares37, k, lo, hi, multisig, nullptr, out_partial);
}

int cbft_bls_combine_finish(cbft_ctx* c, const uint8_t* partials, uint32_t count, uint8_t* out33) {
  c = cbft_dev0(c);
  if (!c || !out33 || !count || !partials) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(c->bls_partial.reserve((size_t)count * CBFT_BLS_G1_PARTIAL_BYTES));
  CBFT_HIP(c->bls_out.reserve(33));
  CBFT_HIP(hipMemcpyAsync(c->bls_partial.p, partials, (size_t)count * CBFT_BLS_G1_PARTIAL_BYTES,
                          hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(cbft_bls_launch_g1_parts(c->bls_partial.as<uint32_t>(), count, c->bls_out.as<uint8_t>(), c->stream));
  CBFT_HIP(hipMemcpyAsync(out33, c->bls_out.p, 33, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  return CBFT_OK;
}

// multisig: the key-sum partials are on the device (c->bls_partial); one fused launch sums them,
// streams the key's lines into the (H, PK) Miller loop and verifies
static int bls_verify_multisig_parts(cbft_ctx* c, uint32_t len, const uint8_t* sig33, uint32_t count, int* out_ok) {
  CBFT_HIP(c->bls_shares.reserve(33));
  CBFT_HIP(c->bls_out.reserve(33));
  CBFT_HIP(hipMemcpyAsync(c->bls_shares.p, sig33, 33, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(cbft_bls_launch_verify_multisig(c->bls_partial.as<uint32_t>(), count, c->bls_msg.as<uint8_t>(), len,
                                           c->bls_shares.as<uint8_t>(), c->bls_gen_lines.as<uint32_t>(),
                                           c->bls_ms_ok.as<uint8_t>(), c->bls_out.as<uint8_t>(), c->stream));
  uint8_t r = 0;
  CBFT_HIP(hipMemcpyAsync(&r, c->bls_out.p, 1, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  *out_ok = r ? 1 : 0;
  return CBFT_OK;
}

// the message is on the device (bls_upload_msg): the verify kernel hashes it itself
static int bls_verify_with_lines(cbft_ctx* c, uint32_t len, const uint8_t* sig33, const uint32_t* d_lines,
                                 const uint8_t* d_ok, int* out_ok) {
  CBFT_HIP(c->bls_shares.reserve(33));
  CBFT_HIP(c->bls_out.reserve(33));
  CBFT_HIP(hipMemcpyAsync(c->bls_shares.p, sig33, 33, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(cbft_bls_launch_verify(c->bls_msg.as<uint8_t>(), len, c->bls_H.as<uint32_t>(), c->bls_shares.as<uint8_t>(),
                                  d_lines, d_ok, c->bls_gen_lines.as<uint32_t>(), c->bls_out.as<uint8_t>(),
                                  c->stream));
  uint8_t r = 0;
  CBFT_HIP(hipMemcpyAsync(&r, c->bls_out.p, 1, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  *out_ok = r ? 1 : 0;
  return CBFT_OK;
}

int cbft_bls_verify(cbft_ctx* c, uint32_t id, const uint8_t* msg, uint32_t len, const uint8_t* sig33, int* out_ok) {
  c = cbft_dev0(c);
  if (!c || !sig33 || !out_ok || (len && !msg)) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  BlsKeySet* ks = find_set(c, id);
  if (!ks) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  int rc = bls_gen_lines(c);
  if (!rc) rc = bls_upload_msg(c, msg, len);
  if (rc) return rc;
  return bls_verify_with_lines(c, len, sig33, ks->lines.as<uint32_t>(), ks->ok.as<uint8_t>(), out_ok);
}

// The SignaturesProcessingJob policy (CollectorOfThresholdSignatures.hpp:363-406) as one call,
// every step on the device with the shares staged and parsed once:
//   optimistic: combine all shares (first share per id), verify the combined signature;
//   otherwise (or optimistic = 0): verify every share, combine the valid ones, verify.
int cbft_bls_combine_threshold(cbft_ctx* c, uint32_t id, const uint8_t* msg, uint32_t len, const uint8_t* shares37,
                               uint32_t k, int optimistic, uint8_t* out_sig33, uint8_t* bad_bitmap, int* out_ok) {
  c = cbft_dev0(c);
  if (!c || !out_sig33 || !out_ok || (k && (!shares37 || !bad_bitmap)) || (len && !msg) || k > BLS_MAX_SHARES)
    return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  BlsKeySet* ks = find_set(c, id);
  if (!ks) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  // the accumulators keep the first share of an id (ThresholdAccumulatorBase::add); later ones
  // are ignored, neither combined nor reported
  std::vector<uint8_t> first(k ? k : 1, 0);
  {
    std::vector<uint8_t> seen(BLS_MAX_SHARES + 1, 0);
    for (uint32_t j = 0; j < k; j++) {
      const uint8_t* sh = shares37 + 37 * (size_t)j;
      const uint32_t sid = ((uint32_t)sh[0] << 24) | ((uint32_t)sh[1] << 16) | ((uint32_t)sh[2] << 8) | sh[3];
      if (sid >= 1 && sid <= BLS_MAX_SHARES) {
        first[j] = seen[sid] ? 0 : 1;
        seen[sid] = 1;
      } else {
        first[j] = 1;  // out of range: fails parse (id check), reported bad
      }
    }
  }
  int rc = bls_gen_lines(c);
  if (!rc) rc = bls_upload_msg(c, msg, len);
  if (!rc && k) rc = bls_prep(c, ks, shares37, k, true, len);  // H beside the shares' decoding
  if (rc) return rc;
  CBFT_HIP(c->bls_first.reserve(k ? k : 1));
  CBFT_HIP(c->bls_use.reserve(k ? k : 1));
  CBFT_HIP(c->bls_lambda.reserve((size_t)(k ? k : 1) * 8 * 4));
  CBFT_HIP(c->bls_partial.reserve((size_t)(2 * k + 16) * BLS_JAC_WORDS * 4));  // row MSM levels
  CBFT_HIP(c->bls_out.reserve(BLS_JAC_WORDS * 4));
  CBFT_HIP(c->bls_flag.reserve(1));
  CBFT_HIP(c->bls_aff.reserve(BLS_SIG_WORDS * 4));
  if (!c->bls_inv.p) {
    CBFT_HIP(c->bls_inv.reserve((size_t)BLS_INV_TABLE * 9 * 4));
    CBFT_HIP(cbft_bls_launch_inv_table(c->bls_inv.as<uint32_t>(), c->stream));
  }
  if (k) CBFT_HIP(hipMemcpyAsync(c->bls_first.p, first.data(), k, hipMemcpyHostToDevice, c->stream));
  // combine over d_use, then verify the device-resident result: result byte -> bls_flag.  The verify
  // takes H from bls_prep (same message, same call) and the combined point in affine form from the
  // combine's finish kernel: no second hash to G1, no decompression before its Miller loops.
  auto combine_verify = [&]() -> int {
    CBFT_HIP(cbft_bls_launch_combine(c->bls_sig.as<uint32_t>(), c->bls_ids.as<uint32_t>(), c->bls_use.as<uint8_t>(),
                                     k, 0, k, 0, c->bls_inv.as<uint32_t>(), c->bls_lambda.as<uint32_t>(),
                                     c->bls_partial.as<uint32_t>(), c->bls_out.as<uint8_t>(), c->bls_aff.as<uint32_t>(),
                                     nullptr, c->stream));
    CBFT_HIP(cbft_bls_launch_verify(c->bls_msg.as<uint8_t>(), len, nullptr, c->bls_out.as<uint8_t>(),
                                    ks->lines.as<uint32_t>(), ks->ok.as<uint8_t>(),
                                    c->bls_gen_lines.as<uint32_t>(), c->bls_flag.as<uint8_t>(), c->stream,
                                    k ? c->bls_H.as<uint32_t>() : nullptr, c->bls_aff.as<uint32_t>()));
    return CBFT_OK;
  };
  std::vector<uint8_t> v(k ? k : 1, 0);
  uint8_t ok = 0, sig33[33] = {0};
  bool done = false;
  if (optimistic && k) {
    CBFT_HIP(cbft_bls_launch_and(c->bls_first.as<uint8_t>(), c->bls_valid.as<uint8_t>(), c->bls_use.as<uint8_t>(), k,
                                 c->stream));
    rc = combine_verify();
    if (rc) return rc;
    CBFT_HIP(hipMemcpyAsync(v.data(), c->bls_valid.p, k, hipMemcpyDeviceToHost, c->stream));
    CBFT_HIP(hipMemcpyAsync(&ok, c->bls_flag.p, 1, hipMemcpyDeviceToHost, c->stream));
    CBFT_HIP(hipMemcpyAsync(sig33, c->bls_out.p, 33, hipMemcpyDeviceToHost, c->stream));
    CBFT_HIP(hipStreamSynchronize(c->stream));
    bool all_parsed = true;
    for (uint32_t j = 0; j < k; j++) all_parsed = all_parsed && (v[j] || !first[j]);
    done = ok && all_parsed;
    if (done) std::memset(bad_bitmap, 0, (k + 7) / 8);
  }
  if (!done) {
    if (k) {
      rc = bls_verify_parsed(c, ks, k);  // verify every decoded share
      if (rc) return rc;
      CBFT_HIP(cbft_bls_launch_and(c->bls_first.as<uint8_t>(), c->bls_valid.as<uint8_t>(), c->bls_use.as<uint8_t>(),
                                   k, c->stream));
    }
    rc = combine_verify();
    if (rc) return rc;
    if (k) CBFT_HIP(hipMemcpyAsync(v.data(), c->bls_valid.p, k, hipMemcpyDeviceToHost, c->stream));
    CBFT_HIP(hipMemcpyAsync(&ok, c->bls_flag.p, 1, hipMemcpyDeviceToHost, c->stream));
    CBFT_HIP(hipMemcpyAsync(sig33, c->bls_out.p, 33, hipMemcpyDeviceToHost, c->stream));
    CBFT_HIP(hipStreamSynchronize(c->stream));
    if (k) std::memset(bad_bitmap, 0, (k + 7) / 8);
    for (uint32_t j = 0; j < k; j++)
      if (first[j] && !v[j]) bad_bitmap[j >> 3] |= (uint8_t)(1u << (j & 7));
  }
  std::memcpy(out_sig33, sig33, 33);  // copied back with the verdicts, before the last synchronisation
  *out_ok = ok ? 1 : 0;
  return CBFT_OK;
}

int cbft_bls_verify_multisig(cbft_ctx* c, uint32_t id, const uint8_t* msg, uint32_t len, const uint8_t* sig33,
                             const uint8_t* signers256, int* out_ok) {
  c = cbft_dev0(c);
  if (!c || !sig33 || !signers256 || !out_ok || (len && !msg)) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  BlsKeySet* ks = find_set(c, id);
  if (!ks) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  int rc = bls_gen_lines(c);
  if (!rc) rc = bls_upload_msg(c, msg, len);
  if (rc) return rc;
  CBFT_HIP(c->bls_bitmap.reserve(256));
  CBFT_HIP(c->bls_ms_ok.reserve(1));
  CBFT_HIP(c->bls_g2tmp.reserve(cbft_bls_g2_sum_tmp_words() * 4));
  CBFT_HIP(c->bls_partial.reserve(CBFT_BLS_G2_PARTIAL_BYTES));
  CBFT_HIP(hipMemcpyAsync(c->bls_bitmap.p, signers256, 256, hipMemcpyHostToDevice, c->stream));
  // PK = sum vk_i (one Jacobian partial), then the fused 3-wave verify (lines streamed into the
  // Miller loop)
  CBFT_HIP(cbft_bls_launch_g2_sum(ks->aff.as<uint32_t>() + BLS_G2A_WORDS, ks->ok.as<uint8_t>() + 1, ks->n,
                                  c->bls_bitmap.as<uint8_t>(), 1, ks->n + 1, c->bls_ms_ok.as<uint8_t>(), nullptr,
                                  c->bls_partial.as<uint32_t>(), c->bls_g2tmp.as<uint32_t>(), c->stream));
  return bls_verify_multisig_parts(c, len, sig33, 1, out_ok);
}

int cbft_bls_sum_keys(cbft_ctx* c, uint32_t id, const uint8_t* signers256, uint8_t* out65) {
  c = cbft_dev0(c);
  if (!c || !signers256 || !out65) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  BlsKeySet* ks = find_set(c, id);
  if (!ks) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(c->bls_bitmap.reserve(256));
  CBFT_HIP(c->bls_ms_ok.reserve(1));
  CBFT_HIP(c->bls_g2tmp.reserve(cbft_bls_g2_sum_tmp_words() * 4));
  CBFT_HIP(c->bls_out.reserve(65));
  CBFT_HIP(hipMemcpyAsync(c->bls_bitmap.p, signers256, 256, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(cbft_bls_launch_g2_sum(ks->aff.as<uint32_t>() + BLS_G2A_WORDS, ks->ok.as<uint8_t>() + 1, ks->n,
                                  c->bls_bitmap.as<uint8_t>(), 1, ks->n + 1, c->bls_ms_ok.as<uint8_t>(),
                                  c->bls_out.as<uint8_t>(), nullptr, c->bls_g2tmp.as<uint32_t>(), c->stream));
  CBFT_HIP(hipMemcpyAsync(out65, c->bls_out.p, 65, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  return CBFT_OK;
}

int cbft_bls_sum_keys_partial(cbft_ctx* c, uint32_t id, const uint8_t* signers256, uint32_t lo_id, uint32_t hi_id,
                              uint8_t* out_partial) {
  c = cbft_dev0(c);
  if (!c || !signers256 || !out_partial || lo_id > hi_id) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  BlsKeySet* ks = find_set(c, id);
  if (!ks) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(c->bls_bitmap.reserve(256));
  CBFT_HIP(c->bls_ms_ok.reserve(1));
  CBFT_HIP(c->bls_g2tmp.reserve(cbft_bls_g2_sum_tmp_words() * 4));
  CBFT_HIP(c->bls_partial.reserve(CBFT_BLS_G2_PARTIAL_BYTES));
  CBFT_HIP(hipMemcpyAsync(c->bls_bitmap.p, signers256, 256, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(cbft_bls_launch_g2_sum(ks->aff.as<uint32_t>() + BLS_G2A_WORDS, ks->ok.as<uint8_t>() + 1, ks->n,
                                  c->bls_bitmap.as<uint8_t>(), lo_id, hi_id, c->bls_ms_ok.as<uint8_t>(), nullptr,
                                  c->bls_partial.as<uint32_t>(), c->bls_g2tmp.as<uint32_t>(), c->stream));
  CBFT_HIP(hipMemcpyAsync(out_partial, c->bls_partial.p, CBFT_BLS_G2_PARTIAL_BYTES, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  return CBFT_OK;
}

int cbft_bls_verify_multisig_partials(cbft_ctx* c, const uint8_t* msg, uint32_t len, const uint8_t* sig33,
                                      const uint8_t* key_partials, uint32_t count, int* out_ok) {
  c = cbft_dev0(c);
  if (!c || !sig33 || !key_partials || !count || !out_ok || (len && !msg)) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  int rc = bls_gen_lines(c);
  if (!rc) rc = bls_upload_msg(c, msg, len);
  if (rc) return rc;
  CBFT_HIP(c->bls_partial.reserve((size_t)count * CBFT_BLS_G2_PARTIAL_BYTES));
  CBFT_HIP(c->bls_ms_ok.reserve(1));
  CBFT_HIP(hipMemcpyAsync(c->bls_partial.p, key_partials, (size_t)count * CBFT_BLS_G2_PARTIAL_BYTES,
                          hipMemcpyHostToDevice, c->stream));
  return bls_verify_multisig_parts(c, len, sig33, count, out_ok);
}

// Clears a host copy of a secret scalar (a volatile store the compiler cannot drop).
static void secure_zero(void* p, size_t n) {
  volatile uint8_t* v = static_cast<volatile uint8_t*>(p);
  while (n--) *v++ = 0;
}

// 32-byte big-endian scalar -> 8 little-endian words
static void be32_scalar_words(uint32_t* w, const uint8_t* sk32) {
  for (int q = 0; q < 8; q++)
    w[q] = ((uint32_t)sk32[31 - 4 * q - 3] << 24) | ((uint32_t)sk32[31 - 4 * q - 2] << 16) |
           ((uint32_t)sk32[31 - 4 * q - 1] << 8) | sk32[31 - 4 * q];
}

// sk mod r in place (r = the BN-P254 group order, 8 little-endian words).  The row kernels take
// k in [1, r): sk * P = (sk mod r) * P for every P of order r, so a key >= r is reduced (at most 6
// subtractions below 2^256); sk = 0 (mod r) is no key and is refused.  Variable time in the
// number of subtractions only for keys >= r, which no key generator produces.
static bool scalar_mod_r(uint32_t* w) {
  static const uint32_t R[8] = {0x0000000d, 0xa1000000, 0x00000010, 0xff9f8000,
                                0x00000007, 0xba344d80, 0x40000001, 0x25236482};
  for (;;) {
    int q = 7;
    while (q >= 0 && w[q] == R[q]) q--;
    if (q >= 0 && w[q] < R[q]) break;  // w < r
    uint64_t borrow = 0;                // w >= r: w -= r
    for (int i = 0; i < 8; i++) {
      const uint64_t d = (uint64_t)w[i] - R[i] - borrow;
      w[i] = (uint32_t)d;
      borrow = (d >> 63) & 1;
    }
  }
  uint32_t any = 0;
  for (int i = 0; i < 8; i++) any |= w[i];
  return any != 0;
}

}  // extern "C"

// the same conversion for the signer tables of cbft_bls_sign.cpp (cbft_internal.h)
bool cbft_bls_scalar_words(uint32_t* w, const uint8_t* sk32) {
  be32_scalar_words(w, sk32);
  return scalar_mod_r(w);
}

extern "C" {

int cbft_bls_public_key(cbft_ctx* c, const uint8_t* sk32, uint8_t* out65) {
  c = cbft_dev0(c);
  if (!c || !sk32 || !out65) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);  // held until the wipe below has run
  uint32_t w[8];
  // every exit, error paths included (the guard exists before the scalar is read): once the
  // scalar went to the device, the stream has finished with it and the device copy is cleared;
  // the host copy is zeroed
  struct Wipe {
    cbft_ctx* c;
    uint32_t* w;
    bool on_device = false;
    bool cleared = false;
    ~Wipe() {
      if (on_device && !cleared) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipMemsetAsync(c->bls_lambda.p, 0, 8 * sizeof(uint32_t), c->stream);
        (void)hipStreamSynchronize(c->stream);
      }
      secure_zero(w, 8 * sizeof(uint32_t));
    }
  } wipe{c, w};
  be32_scalar_words(w, sk32);
  if (!scalar_mod_r(w)) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(c->bls_lambda.reserve(8 * 4));
  CBFT_HIP(c->bls_out.reserve(65));
  wipe.on_device = true;
  CBFT_HIP(hipMemcpyAsync(c->bls_lambda.p, w, sizeof(w), hipMemcpyHostToDevice, c->stream));
  // fixed-base comb of g2 on row-parallel Fp (its 64 x 8 table built once per context, ~10 ms)
  if (!c->bls_pub_tbl.p) {
    CBFT_HIP(c->bls_pub_tbl.reserve(cbft_bls_pub_table_words() * sizeof(uint32_t)));
    CBFT_HIP(cbft_bls_launch_pub_table(c->bls_pub_tbl.as<uint32_t>(), c->stream));
  }
  CBFT_HIP(cbft_bls_launch_pubkey_row(c->bls_pub_tbl.as<uint32_t>(), c->bls_lambda.as<uint32_t>(),
                                      c->bls_out.as<uint8_t>(), c->stream));
  CBFT_HIP(hipMemcpyAsync(out65, c->bls_out.p, 65, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipMemsetAsync(c->bls_lambda.p, 0, sizeof(w), c->stream));  // the secret scalar leaves the device
  CBFT_HIP(hipStreamSynchronize(c->stream));
  wipe.cleared = true;
  return CBFT_OK;
}

int cbft_bls_sign(cbft_ctx* c, const uint8_t* sk32, uint32_t id, const uint8_t* msg, uint32_t len, uint8_t* out37) {
  c = cbft_dev0(c);
  if (!c || !sk32 || !out37 || (len && !msg)) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);  // held until the wipe below has run
  uint32_t w[8];
  const size_t msg_at = sizeof(w);
  std::vector<uint8_t> in(msg_at + len);  // alive (and the scalar in it) until the stream is done
  // every exit, error paths included (the wipe exists before the scalar is read): once the
  // scalar went to the device, the stream has finished reading `in` and the device copy is
  // cleared; both host copies are zeroed
  struct Wipe {
    cbft_ctx* c;
    uint32_t* w;
    std::vector<uint8_t>& in;
    bool on_device = false;  // an H2D of the scalar was queued
    bool cleared = false;    // the success path queued the device clear and synchronised
    ~Wipe() {
      if (on_device && !cleared) {
        (void)hipStreamSynchronize(c->stream);
        if (c->bls_msg.p) {
          (void)hipMemsetAsync(c->bls_msg.p, 0, 8 * sizeof(uint32_t), c->stream);
          (void)hipStreamSynchronize(c->stream);
        }
      }
      secure_zero(w, 8 * sizeof(uint32_t));
      secure_zero(in.data(), in.size() < 32 ? in.size() : 32);
    }
  } wipe{c, w, in};
  be32_scalar_words(w, sk32);
  if (!scalar_mod_r(w)) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  // one H2D: the scalar's words, then the message (bls_msg = [sk words | msg])
  CBFT_HIP(c->bls_msg.reserve(msg_at + len + 1));
  CBFT_HIP(c->bls_out.reserve(37));
  std::memcpy(in.data(), w, sizeof(w));
  if (len) std::memcpy(in.data() + msg_at, msg, len);
  wipe.on_device = true;
  CBFT_HIP(hipMemcpyAsync(c->bls_msg.p, in.data(), in.size(), hipMemcpyHostToDevice, c->stream));
  const uint32_t* d_sk = c->bls_msg.as<uint32_t>();
  const uint8_t* d_msg = c->bls_msg.as<uint8_t>() + msg_at;
  // row-parallel GLV signature (0.4-0.5 ms), the hash to G1 inside the signing kernel (H = nullptr)
  CBFT_HIP(cbft_bls_launch_sign_row(nullptr, d_sk, d_msg, len, id, c->bls_out.as<uint8_t>(), c->stream));
  CBFT_HIP(hipMemcpyAsync(out37, c->bls_out.p, 37, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipMemsetAsync(c->bls_msg.p, 0, sizeof(w), c->stream));  // the secret scalar leaves the device
  CBFT_HIP(hipStreamSynchronize(c->stream));
  wipe.cleared = true;  // (Wipe zeroes the host copies)
  return CBFT_OK;
}

}  // extern "C"
