// libcbft_hipcrypto, batched BLS multisig verification half of the C ABI (include/cbft_hipcrypto.h).
//
// The batch form of BlsMultisigVerifier::verify for k-of-n keys (the reference generates multisig-bls
// keys): a view change, a checkpoint or a replica with a window of sequence numbers open holds many
// (digest, sigma, signer bitmap) triples at once.  One call takes s signer bitmaps, m messages and n
// items, each naming its set (set_of) and its message (msg_of), sums each set's keys once and gives n
// exact verdicts (bls_multisig_batch.hip).  cbft_bls_verify_multisig stays the one-certificate call.
//
// Multi-GPU contexts: the host form cuts the items into contiguous slices, one per device, each
// summing only the sets and hashing only the messages its slice names; the _device entry needs a
// single-GPU context.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "bls_kernels.h"
#include "bls_multisig_batch.h"
#include "cbft_internal.h"

static_assert(BLS_MULTISIG_MAX_SETS == CBFT_BLS_MULTISIG_MAX_SETS, "set cap of the header");

void cbft_bls_multisig_batch_release(cbft_ctx* c) {
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();  // device-path batches run on caller streams
  for (DevBuf* b : {&c->blsm.in, &c->blsm.sets, &c->blsm.out}) b->release();
  c->blsm.scratch.release();
}

// the argument checks of the host form that need no device: CBFT_EINVAL before anything is launched
static int blsm_check(size_t s, const uint32_t* set_of, const uint32_t* msg_len, size_t m, const uint32_t* msg_of,
                      size_t n) {
  if ((!set_of && s != n) || (!msg_of && m != n)) return CBFT_EINVAL;
  for (size_t j = 0; j < m; j++)
    if (msg_len[j] > CBFT_MAX_MSG_LEN) return CBFT_EINVAL;
  for (size_t i = 0; i < n; i++) {
    if (set_of && set_of[i] >= s) return CBFT_EINVAL;
    if (msg_of && msg_of[i] >= m) return CBFT_EINVAL;
  }
  return CBFT_OK;
}

static void blsm_keys(cbft_ctx* c, BlsKeySet& ks, BlsMultisigBatch& b) {
  b.nkeys = ks.n;
  b.aff = ks.aff.as<uint32_t>();
  b.key_ok = ks.ok.as<uint8_t>();
  b.gen_lines = c->bls_gen_lines.as<uint32_t>();
}

static int blsm_launch_locked(cbft_ctx* c, BlsKeySet& ks, BlsMultisigBatch b, uint8_t* d_valid, hipStream_t s) {
  if (!c->bls_gen_lines.p) return CBFT_EINVAL;  // built by cbft_bls_load_keys: a key set implies them
  blsm_keys(c, ks, b);
  CBFT_HIP(c->blsm.scratch.acquire(cbft_bls_multisig_batch_scratch_bytes(b.n, b.m, b.s, b.nkeys), s));
  CBFT_HIP(cbft_bls_multisig_batch_launch(b, c->blsm.scratch.buf.p, d_valid, s));
  CBFT_HIP(c->blsm.scratch.commit(s));
  return CBFT_OK;
}

// one device, host arrays: n verdict bytes into out (0 / 1)
static int blsm_host_one(cbft_ctx* c, uint32_t id, const uint8_t* signers256, size_t s, const uint32_t* set_of,
                         const uint8_t* sig33, const uint8_t* msg_blob, const uint64_t* msg_off,
                         const uint32_t* msg_len, size_t m, const uint32_t* msg_of, size_t n, uint8_t* out) {
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->bls_sets.find(id);
  if (it == c->bls_sets.end()) return CBFT_EINVAL;
  const int rc0 = blsm_check(s, set_of, msg_len, m, msg_of, n);
  if (rc0) return rc0;
  if (s > BLS_MULTISIG_MAX_SETS) return CBFT_E2BIG;  // after every CBFT_EINVAL check
  if (n == 0) return CBFT_OK;
  // no length cap here: blsm_check has applied it
  c->host_off.resize(m);
  const CbftSpan span = cbft_msg_span(msg_off, msg_len, m, 0, msg_blob != nullptr, c->host_off.data());
  if (span.err) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  // the packed image's middle arrays: set indices | message indices | signatures; the bitmaps beside it
  const CbftPackedArray mid[3] = {{set_of, n * 4}, {msg_of, n * 4}, {sig33, n * 33}};
  CbftPackedLayout L;
  CBFT_HIP(cbft_upload_packed(c->blsm.in, c->stream, c->host_off.data(), msg_len, m, mid, 3, msg_blob, span, &L));
  CBFT_HIP(c->blsm.sets.reserve(s * 256));
  CBFT_HIP(hipMemcpyAsync(c->blsm.sets.p, signers256, s * 256, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(c->blsm.out.reserve(n));
  const uint8_t* d = c->blsm.in.as<uint8_t>();
  BlsMultisigBatch b{};
  b.n = (uint32_t)n;
  b.m = (uint32_t)m;
  b.s = (uint32_t)s;
  b.signers = c->blsm.sets.as<uint8_t>();
  b.set_of = set_of ? reinterpret_cast<const uint32_t*>(d + L.mid[0]) : nullptr;
  b.msg_of = msg_of ? reinterpret_cast<const uint32_t*>(d + L.mid[1]) : nullptr;
  b.sig33 = d + L.mid[2];
  b.msg = d + L.blob;
  b.off = reinterpret_cast<const uint64_t*>(d + L.off);
  b.len = reinterpret_cast<const uint32_t*>(d + L.len);
  const int rc = blsm_launch_locked(c, it->second, b, c->blsm.out.as<uint8_t>(), c->stream);
  if (rc) return rc;
  CBFT_HIP(hipMemcpyAsync(out, c->blsm.out.p, n, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  return CBFT_OK;
}

static void blsm_pack(uint8_t* bitmap, const uint8_t* v, size_t n) {
  std::memset(bitmap, 0, (n + 7) / 8);
  for (size_t j = 0; j < n; j++)
    if (v[j]) bitmap[j >> 3] |= (uint8_t)(1u << (j & 7));
}

extern "C" {

int cbft_bls_verify_multisig_batch(cbft_ctx* c, uint32_t id, const uint8_t* signers256, size_t s,
                                   const uint32_t* set_of, const uint8_t* sig33, const uint8_t* msg_blob,
                                   const uint64_t* msg_off, const uint32_t* msg_len, size_t m, const uint32_t* msg_of,
                                   size_t n, uint8_t* valid_bitmap) {
  if (!c || (n && (!sig33 || !valid_bitmap)) || (m && (!msg_off || !msg_len)) || (s && !signers256)) return CBFT_EINVAL;
  if (n > BLS_VERIFY_BATCH_MAX || m > BLS_VERIFY_BATCH_MAX) return CBFT_E2BIG;
  std::vector<uint8_t> v(n);
  if (c->kids.empty()) {
    const int rc = blsm_host_one(c, id, signers256, s, set_of, sig33, msg_blob, msg_off, msg_len, m, msg_of, n, v.data());
    if (rc || !n) return rc;
    blsm_pack(valid_bitmap, v.data(), n);
    return CBFT_OK;
  }
  // multi-GPU: every check before any device starts, then one contiguous slice of items per device
  {
    cbft_ctx* k0 = c->kids[0];
    std::lock_guard<std::mutex> g(k0->mu);
    if (k0->bls_sets.find(id) == k0->bls_sets.end()) return CBFT_EINVAL;
    const int rc0 = blsm_check(s, set_of, msg_len, m, msg_of, n);
    if (rc0 || !n) return rc0;
  }
  const size_t G = c->kids.size(), per = (n + G - 1) / G;
  // the sets and the messages each slice names, renumbered in order of first use
  struct Slice {
    std::vector<uint8_t> sets;
    std::vector<uint32_t> sof, mof, len;
    std::vector<uint64_t> off;
  };
  std::vector<Slice> sl(G);
  for (size_t g = 0; g < G; g++) {
    const size_t lo = std::min(n, g * per), hi = std::min(n, lo + per), cnt = hi - lo;
    Slice& x = sl[g];
    std::vector<uint32_t> ls(s, UINT32_MAX), lm(m, UINT32_MAX);
    x.sof.resize(cnt);
    x.mof.resize(cnt);
    for (size_t i = 0; i < cnt; i++) {
      const uint32_t j = set_of ? set_of[lo + i] : (uint32_t)(lo + i);
      if (ls[j] == UINT32_MAX) {
        ls[j] = (uint32_t)(x.sets.size() / 256);
        x.sets.insert(x.sets.end(), signers256 + 256 * (size_t)j, signers256 + 256 * (size_t)j + 256);
      }
      x.sof[i] = ls[j];
      const uint32_t k = msg_of ? msg_of[lo + i] : (uint32_t)(lo + i);
      if (lm[k] == UINT32_MAX) {
        lm[k] = (uint32_t)x.off.size();
        x.off.push_back(msg_off[k]);
        x.len.push_back(msg_len[k]);
      }
      x.mof[i] = lm[k];
    }
    if (x.sets.size() / 256 > BLS_MULTISIG_MAX_SETS) return CBFT_E2BIG;
  }
  const int rc = for_each_kid(c, [&](size_t g) {
    const size_t lo = std::min(n, g * per), hi = std::min(n, lo + per), cnt = hi - lo;
    if (!cnt) return (int)CBFT_OK;
    Slice& x = sl[g];
    return blsm_host_one(c->kids[g], id, x.sets.data(), x.sets.size() / 256, x.sof.data(), sig33 + 33 * lo, msg_blob,
                         x.off.data(), x.len.data(), x.off.size(), x.mof.data(), cnt, v.data() + lo);
  });
  if (rc) return rc;
  blsm_pack(valid_bitmap, v.data(), n);
  return CBFT_OK;
}

int cbft_bls_verify_multisig_fixed_device(cbft_ctx* c, uint32_t id, const uint8_t* d_signers256, size_t s,
                                          const uint32_t* d_set_of, const uint8_t* d_sig33, const uint8_t* d_msg,
                                          uint32_t msg_len, size_t m, const uint32_t* d_msg_of, size_t n,
                                          uint8_t* d_valid, void* stream) {
  if (c && !c->kids.empty()) return CBFT_EINVAL;  // device pointers belong to one GPU: use its own context
  if (!c || (n && (!d_sig33 || !d_valid)) || (m && msg_len && !d_msg) || (s && !d_signers256)) return CBFT_EINVAL;
  if (msg_len > CBFT_MAX_MSG_LEN || (!d_msg_of && m != n) || (!d_set_of && s != n)) return CBFT_EINVAL;
  if (n > BLS_VERIFY_BATCH_MAX || m > BLS_VERIFY_BATCH_MAX) return CBFT_E2BIG;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->bls_sets.find(id);
  if (it == c->bls_sets.end()) return CBFT_EINVAL;
  if (s > BLS_MULTISIG_MAX_SETS) return CBFT_E2BIG;
  if (n == 0) return CBFT_OK;
  CBFT_HIP(hipSetDevice(c->device));
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
  BlsMultisigBatch b{};
  b.n = (uint32_t)n;
  b.m = (uint32_t)m;
  b.s = (uint32_t)s;
  b.signers = d_signers256;
  b.set_of = d_set_of;
  b.msg_of = d_msg_of;
  b.sig33 = d_sig33;
  b.msg = d_msg;
  b.fixed_len = msg_len;
  return blsm_launch_locked(c, it->second, b, d_valid, st);
}

int cbft_bls_sum_keys_batch(cbft_ctx* c, uint32_t id, const uint8_t* signers256, size_t s, uint8_t* out65, uint8_t* ok) {
  c = cbft_dev0(c);
  if (!c || (s && (!signers256 || !out65 || !ok))) return CBFT_EINVAL;
  if (s > BLS_MULTISIG_MAX_SETS) return CBFT_E2BIG;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->bls_sets.find(id);
  if (it == c->bls_sets.end()) return CBFT_EINVAL;
  if (s == 0) return CBFT_OK;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(c->blsm.sets.reserve(s * 256));
  CBFT_HIP(hipMemcpyAsync(c->blsm.sets.p, signers256, s * 256, hipMemcpyHostToDevice, c->stream));
  CBFT_HIP(c->blsm.out.reserve(s * 66));
  BlsMultisigBatch b{};
  b.s = (uint32_t)s;
  b.signers = c->blsm.sets.as<uint8_t>();
  blsm_keys(c, it->second, b);
  CBFT_HIP(c->blsm.scratch.acquire(cbft_bls_multisig_sum_scratch_bytes(s, b.nkeys), c->stream));
  uint8_t* d_out = c->blsm.out.as<uint8_t>();
  CBFT_HIP(cbft_bls_multisig_sum_launch(b, c->blsm.scratch.buf.p, d_out, d_out + 65 * s, c->stream));
  CBFT_HIP(c->blsm.scratch.commit(c->stream));
  CBFT_HIP(hipMemcpyAsync(out65, d_out, 65 * s, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipMemcpyAsync(ok, d_out + 65 * s, s, hipMemcpyDeviceToHost, c->stream));
  CBFT_HIP(hipStreamSynchronize(c->stream));
  return CBFT_OK;
}

}  // extern "C"
