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
  for (DevBuf* b : {&c->blsv.in, &c->blsv.out}) b->release();
  c->blsv.scratch.release();
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
  CBFT_HIP(c->blsv.scratch.acquire(cbft_bls_verify_batch_scratch_bytes(b.n, b.m), s));
  b.nkeys = ks.n;
  b.lines = ks.lines.as<uint32_t>();
  b.key_ok = ks.ok.as<uint8_t>();
  b.gen_lines = c->bls_gen_lines.as<uint32_t>();
  CBFT_HIP(cbft_bls_verify_batch_launch(b, c->blsv.scratch.buf.p, d_valid, s));
  CBFT_HIP(c->blsv.scratch.commit(s));
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
  // no length cap here: blsv_check has applied it
  c->host_off.resize(m);
  const CbftSpan span = cbft_msg_span(msg_off, msg_len, m, 0, msg_blob != nullptr, c->host_off.data());
  if (span.err) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  // the packed image's middle arrays: key slots | message indices | signatures
  const CbftPackedArray mid[3] = {{key_idx, n * 4}, {msg_of, n * 4}, {sig33, n * 33}};
  CbftPackedLayout L;
  CBFT_HIP(cbft_upload_packed(c->blsv.in, c->stream, c->host_off.data(), msg_len, m, mid, 3, msg_blob, span, &L));
  CBFT_HIP(c->blsv.out.reserve(n));
  const uint8_t* d = c->blsv.in.as<uint8_t>();
  BlsVerifyBatch b{};
  b.n = (uint32_t)n;
  b.m = (uint32_t)m;
  b.key_idx = key_idx ? reinterpret_cast<const uint32_t*>(d + L.mid[0]) : nullptr;
  b.msg_of = msg_of ? reinterpret_cast<const uint32_t*>(d + L.mid[1]) : nullptr;
  b.sig33 = d + L.mid[2];
  b.msg = d + L.blob;
  b.off = reinterpret_cast<const uint64_t*>(d + L.off);
  b.len = reinterpret_cast<const uint32_t*>(d + L.len);
  const int rc = blsv_launch_locked(c, it->second, b, c->blsv.out.as<uint8_t>(), c->stream);
  if (rc) return rc;
  CBFT_HIP(hipMemcpyAsync(out, c->blsv.out.p, n, hipMemcpyDeviceToHost, c->stream));
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
