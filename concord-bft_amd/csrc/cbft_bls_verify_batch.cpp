// libcbft_hipcrypto, batched BLS verification half of the C ABI (include/cbft_hipcrypto.h).
//
// The batch form of IThresholdVerifier::verify and of the accumulators' share check: every replica
// that is not the collector checks one combined signature per sequence number (PrepareFullMsg,
// CommitFullMsg, FullCommitProofMsg), a view change or a checkpoint presents many certificates at
// once, and a collector with a window of sequence numbers open holds shares of many digests.  One
// call takes n items, each with its own message (msg_of, so that the shares of one digest hash it
// once) and its own key slot (0 = the group PK, i = vk_i), and gives n exact verdicts
// (bls_verify_batch.hip).  cbft_bls_verify and cbft_bls_verify_shares stay the one-message calls.
//
// Multi-GPU contexts: the host form cuts the items into contiguous slices, one per device, each
// hashing only the messages its slice names; the _device entry needs a single-GPU context.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "bls_kernels.h"
#include "bls_verify_batch.h"
#include "cbft_internal.h"

void cbft_bls_verify_batch_release(cbft_ctx* c) {
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();  // device-path batches run on caller streams
  for (DevBuf* b : {&c->blsv_scratch, &c->blsv_in, &c->blsv_out}) b->release();
  if (c->blsv_done) (void)hipEventDestroy(c->blsv_done);
  c->blsv_done = nullptr;
  c->blsv_used = false;
}

// the argument checks of the host form that need no device: CBFT_EINVAL before anything is launched
static int blsv_check(uint32_t nkeys, const uint32_t* key_idx, const uint32_t* msg_len, size_t m,
                      const uint32_t* msg_of, size_t n) {
  if (!msg_of && m != n) return CBFT_EINVAL;
  for (size_t j = 0; j < m; j++)
    if (msg_len[j] > CBFT_MAX_MSG_LEN) return CBFT_EINVAL;
  for (size_t i = 0; i < n; i++) {
    if (key_idx && key_idx[i] > nkeys) return CBFT_EINVAL;
    if (msg_of && msg_of[i] >= m) return CBFT_EINVAL;
  }
  return CBFT_OK;
}

static int blsv_launch_locked(cbft_ctx* c, BlsKeySet& ks, BlsVerifyBatch b, uint8_t* d_valid, hipStream_t s) {
  if (!c->bls_gen_lines.p) return CBFT_EINVAL;  // built by cbft_bls_load_keys: a key set implies them
  CBFT_HIP(c->blsv_scratch.reserve(cbft_bls_verify_batch_scratch_bytes(b.n, b.m)));
  if (!c->blsv_done) CBFT_HIP(hipEventCreateWithFlags(&c->blsv_done, hipEventDisableTiming));
  if (c->blsv_used) CBFT_HIP(hipStreamWaitEvent(s, c->blsv_done, 0));  // scratch reuse across streams
  b.nkeys = ks.n;
  b.lines = ks.lines.as<uint32_t>();
  b.key_ok = ks.ok.as<uint8_t>();
  b.gen_lines = c->bls_gen_lines.as<uint32_t>();
  CBFT_HIP(cbft_bls_verify_batch_launch(b, c->blsv_scratch.p, d_valid, s));
  CBFT_HIP(hipEventRecord(c->blsv_done, s));
  c->blsv_used = true;
  return CBFT_OK;
}

// one device, host arrays: n verdict bytes into out (0 / 1)
static int blsv_host_one(cbft_ctx* c, uint32_t id, const uint32_t* key_idx, const uint8_t* sig33,
                         const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len, size_t m,
                         const uint32_t* msg_of, size_t n, uint8_t* out) {
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->bls_sets.find(id);
  if (it == c->bls_sets.end()) return CBFT_EINVAL;
  const int rc0 = blsv_check(it->second.n, key_idx, msg_len, m, msg_of, n);
  if (rc0) return rc0;
  if (n == 0) return CBFT_OK;
  // the batch's messages are the blob range [lo, hi) their offsets span: only that range moves
  uint64_t lo = UINT64_MAX, hi = 0;
  for (size_t j = 0; j < m; j++) {
    lo = std::min<uint64_t>(lo, msg_off[j]);
    hi = std::max<uint64_t>(hi, msg_off[j] + msg_len[j]);
  }
  if (hi > lo && !msg_blob) return CBFT_EINVAL;
  const uint64_t blob = hi > lo ? hi - lo : 0;
  // one packed device image: offsets (rebased) | lengths | key slots | message indices | signatures | blob
  const size_t o_off = 0, o_len = m * 8, o_key = o_len + m * 4, o_mof = o_key + n * 4, o_sig = o_mof + n * 4,
               o_blob = o_sig + n * 33;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(c->blsv_in.reserve(o_blob + blob + 16));
  CBFT_HIP(c->blsv_out.reserve(n));
  c->host_off.resize(m);
  for (size_t j = 0; j < m; j++) c->host_off[j] = msg_off[j] - lo;
  uint8_t* d = c->blsv_in.as<uint8_t>();
  CBFT_HIP(hipMemcpyAsync(d + o_off, c->host_off.data(), m * 8, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(hipMemcpyAsync(d + o_len, msg_len, m * 4, hipMemcpyHostToDevice, c->stream));
  if (key_idx) CBFT_HIP(hipMemcpyAsync(d + o_key, key_idx, n * 4, hipMemcpyHostToDevice, c->stream));
  if (msg_of) CBFT_HIP(hipMemcpyAsync(d + o_mof, msg_of, n * 4, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(hipMemcpyAsync(d + o_sig, sig33, n * 33, hipMemcpyHostToDevice, c->stream));
  if (blob) CBFT_HIP(hipMemcpyAsync(d + o_blob, msg_blob + lo, blob, hipMemcpyHostToDevice, c->stream));
  BlsVerifyBatch b{};
  b.n = (uint32_t)n;
  b.m = (uint32_t)m;
  b.key_idx = key_idx ? reinterpret_cast<const uint32_t*>(d + o_key) : nullptr;
  b.msg_of = msg_of ? reinterpret_cast<const uint32_t*>(d + o_mof) : nullptr;
  b.sig33 = d + o_sig;
  b.msg = d + o_blob;
  b.off = reinterpret_cast<const uint64_t*>(d + o_off);
  b.len = reinterpret_cast<const uint32_t*>(d + o_len);
  const int rc = blsv_launch_locked(c, it->second, b, c->blsv_out.as<uint8_t>(), c->stream);
  if (rc) return rc;
  CBFT_HIP(hipMemcpyAsync(out, c->blsv_out.p, n, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  return CBFT_OK;
}

static void blsv_pack(uint8_t* bitmap, const uint8_t* v, size_t n) {
  std::memset(bitmap, 0, (n + 7) / 8);
  for (size_t j = 0; j < n; j++)
    if (v[j]) bitmap[j >> 3] |= (uint8_t)(1u << (j & 7));
}

extern "C" {

int cbft_bls_verify_batch(cbft_ctx* c, uint32_t id, const uint32_t* key_idx, const uint8_t* sig33,
                          const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len, size_t m,
                          const uint32_t* msg_of, size_t n, uint8_t* valid_bitmap) {
  if (!c || (n && (!sig33 || !valid_bitmap)) || (m && (!msg_off || !msg_len))) return CBFT_EINVAL;
  if (n > BLS_VERIFY_BATCH_MAX || m > BLS_VERIFY_BATCH_MAX) return CBFT_E2BIG;
  std::vector<uint8_t> v(n);
  if (c->kids.empty()) {
    const int rc = blsv_host_one(c, id, key_idx, sig33, msg_blob, msg_off, msg_len, m, msg_of, n, v.data());
    if (rc || !n) return rc;
    blsv_pack(valid_bitmap, v.data(), n);
    return CBFT_OK;
  }
  // multi-GPU: every check before any device starts, then one contiguous slice of items per device
  {
    cbft_ctx* k0 = c->kids[0];
    std::lock_guard<std::mutex> g(k0->mu);
    auto it = k0->bls_sets.find(id);
    if (it == k0->bls_sets.end()) return CBFT_EINVAL;
    const int rc0 = blsv_check(it->second.n, key_idx, msg_len, m, msg_of, n);
    if (rc0 || !n) return rc0;
  }
  const size_t G = c->kids.size(), per = (n + G - 1) / G;
  const int rc = for_each_kid(c, [&](size_t g) {
    const size_t lo = std::min(n, g * per), hi = std::min(n, lo + per), cnt = hi - lo;
    if (!cnt) return (int)CBFT_OK;
    const uint32_t* ki = key_idx ? key_idx + lo : nullptr;
    if (!msg_of)  // item i signs message i: the slice's messages are its own range
      return blsv_host_one(c->kids[g], id, ki, sig33 + 33 * lo, msg_blob, msg_off + lo, msg_len + lo, cnt, nullptr, cnt,
                           v.data() + lo);
    // the messages this slice names, in order of first use
    std::vector<uint32_t> local(m, UINT32_MAX), mof(cnt), len;
    std::vector<uint64_t> off;
    for (size_t i = 0; i < cnt; i++) {
      const uint32_t j = msg_of[lo + i];
      if (local[j] == UINT32_MAX) {
        local[j] = (uint32_t)off.size();
        off.push_back(msg_off[j]);
        len.push_back(msg_len[j]);
      }
      mof[i] = local[j];
    }
    return blsv_host_one(c->kids[g], id, ki, sig33 + 33 * lo, msg_blob, off.data(), len.data(), off.size(), mof.data(),
                         cnt, v.data() + lo);
  });
  if (rc) return rc;
  blsv_pack(valid_bitmap, v.data(), n);
  return CBFT_OK;
}

int cbft_bls_verify_fixed_device(cbft_ctx* c, uint32_t id, const uint32_t* d_key_idx, const uint8_t* d_sig33,
                                 const uint8_t* d_msg, uint32_t msg_len, size_t m, const uint32_t* d_msg_of, size_t n,
                                 uint8_t* d_valid, void* stream) {
  if (c && !c->kids.empty()) return CBFT_EINVAL;  // device pointers belong to one GPU: use its own context
  if (!c || (n && (!d_sig33 || !d_valid)) || (m && msg_len && !d_msg)) return CBFT_EINVAL;
  if (msg_len > CBFT_MAX_MSG_LEN || (!d_msg_of && m != n)) return CBFT_EINVAL;
  if (n > BLS_VERIFY_BATCH_MAX || m > BLS_VERIFY_BATCH_MAX) return CBFT_E2BIG;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->bls_sets.find(id);
  if (it == c->bls_sets.end()) return CBFT_EINVAL;
  if (n == 0) return CBFT_OK;
  CBFT_HIP(hipSetDevice(c->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  BlsVerifyBatch b{};
  b.n = (uint32_t)n;
  b.m = (uint32_t)m;
  b.key_idx = d_key_idx;
  b.msg_of = d_msg_of;
  b.sig33 = d_sig33;
  b.msg = d_msg;
  b.fixed_len = msg_len;
  return blsv_launch_locked(c, it->second, b, d_valid, s);
}

}  // extern "C"
