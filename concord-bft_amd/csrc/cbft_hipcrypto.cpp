// libcbft_hipcrypto: host side of the C ABI declared in include/cbft_hipcrypto.h.
//
// One context = one GPU + one HIP stream + grow-on-demand device work buffers + the loaded key
// tables.  Calls on a context are serialised by a mutex (the reference calls verifiers
// concurrently from its RequestThreadPool under a shared_lock, SigManager.cpp:203; a caller
// that wants concurrency opens one context per thread or per GPU).
#include "cbft_hipcrypto.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

#include "cbft_internal.h"
#include "ed25519_verify.h"

// Last failure of this thread, for cbft_last_error() (diagnostics only).
static thread_local char g_last_error[256];

int cbft_fail(hipError_t e, const char* what, const char* file, int line) {
  snprintf(g_last_error, sizeof g_last_error, "%s failed at %s:%d: %s (%d)", what, file, line, hipGetErrorString(e),
           (int)e);
  (void)hipGetLastError();
  return e == hipErrorOutOfMemory ? CBFT_ENOMEM : CBFT_EIO;
}

// table-build lanes per launch (bounds the projective staging buffer: 18 KB per lane)
static const size_t kCombBuildLanes = 262144;  // 4 waves per SIMD; 4.7 GB of staging

// comb radix of a key table: explicit (8..15), else $CBFT_COMB_RADIX, else the widest radix
// whose tables for nkeys keys fit the per-table budget ($CBFT_COMB_BUDGET_GB, default 64 GB of
// the 288 GB HBM): 13 (10.5 MB/key, 9 additions per lane) up to ~6,100 keys, 11 (3.0 MB/key,
// 10) up to ~21,000, then 8 (0.53 MB/key, 12).
// HBM a table of nkeys keys takes at radix r: keys live in whole CBFT_KEY_CHUNK-key chunks (comb
// tables + raw keys + decode status), so even one key costs a whole chunk.
static double table_bytes(uint64_t nkeys, int r) {
  const uint64_t chunks = (nkeys + CBFT_KEY_CHUNK - 1) / CBFT_KEY_CHUNK;
  return (double)chunks * (double)cbft_key_chunk_bytes(cbft_comb_geom(r).words_per_unit());
}

static int key_radix(int requested, uint32_t nkeys) {
  if (requested) return requested;
  if (const char* e = getenv("CBFT_COMB_RADIX")) {
    const int r = atoi(e);
    if (r >= 8 && r <= 15) return r;
  }
  double budget = 64.0;
  if (const char* e = getenv("CBFT_COMB_BUDGET_GB")) budget = atof(e);
  // (14 and 15 only on request: at 4,096 keys radix 15's 146 GB of tables saves 3 of 32 additions
  // but its entry reads miss the TLB more, and the pair ladder took 139 us against 110 at 13)
  for (int r : {13, 11}) {
    if (table_bytes(nkeys, r) <= budget * 1e9) return r;
  }
  return 8;
}

// Build comb tables for nunits encoded points (d_pk, 32 B each) into d_tbl, in launches of at
// most kCombBuildLanes lanes (B's radix-2^22 table is 196,608 lanes, 4,096 radix-2^13 keys
// 2.6 M); synchronous.
static hipError_t build_comb(const uint8_t* d_pk, size_t nunits, int negate, const CombGeom& g, uint32_t* d_tbl,
                             uint8_t* d_aok, hipStream_t s) {
  const size_t lanes = nunits * (size_t)g.npos * g.chunks();
  const size_t step = std::min(lanes, kCombBuildLanes);
  DevBuf tmp, pos;
  hipError_t e = tmp.reserve(cbft_ed25519_comb_tmp_words(step) * sizeof(uint32_t));
  if (e == hipSuccess) e = pos.reserve(cbft_ed25519_comb_pos_words(nunits, g) * sizeof(uint32_t));
  if (e == hipSuccess) e = cbft_ed25519_launch_comb_pos(d_pk, nunits, negate, g, pos.as<uint32_t>(), d_aok, s);
  for (size_t l0 = 0; e == hipSuccess && l0 < lanes; l0 += step)
    e = cbft_ed25519_launch_comb_tables(pos.as<uint32_t>(), nunits, g, d_tbl, nullptr, 0, tmp.as<uint32_t>(), l0,
                                        std::min(step, lanes - l0), s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  tmp.release();
  pos.release();
  return e;
}

static int collect_locked(HostSlot& s);

// Comb table of B at radix c->b_radix (the "key" is B's encoding, not negated); synchronous.
static int build_base_comb(cbft_ctx* c) {
  static const uint8_t kB[32] = {0x58, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66,
                                 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66,
                                 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66};
  const CombGeom gb = cbft_comb_geom(c->b_radix);
  DevBuf enc;
  if (c->base_comb.reserve(gb.words_per_unit() * 4) != hipSuccess || enc.reserve(32) != hipSuccess) {
    enc.release();
    return CBFT_ENOMEM;
  }
  const bool ok = hipMemcpy(enc.p, kB, 32, hipMemcpyHostToDevice) == hipSuccess &&
                  build_comb(enc.as<uint8_t>(), 1, 0, gb, c->base_comb.as<uint32_t>(), nullptr, c->stream) == hipSuccess;
  enc.release();
  return ok ? CBFT_OK : CBFT_EIO;
}

// A multi-GPU context runs BLS, RSA and profiling calls on its first device.
cbft_ctx* cbft_dev0(cbft_ctx* c) { return (c && !c->kids.empty()) ? c->kids[0] : c; }

#define CBFT_PROF_RING 256  // batches whose stage events profiling mode 2 keeps

static int reserve_slot(WorkSlot& w, size_t n) {
  CBFT_HIP(w.h.reserve(n * 8 * sizeof(uint32_t)));
  CBFT_HIP(w.flags.reserve(n));
  CBFT_HIP(w.xyz.reserve(n * 27 * sizeof(uint32_t)));
  if (!w.done) CBFT_HIP(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
  return CBFT_OK;
}

// Only the slots launches rotate over (slot 0 also serves small batches): the rest of the
// CBFT_MAX_WORK_SLOTS array stays unallocated.
static int reserve_work(cbft_ctx* c, size_t n) {
  for (int k = 0; k < c->work_slots; k++) {
    int rc = reserve_slot(c->slots[k], n);
    if (rc) return rc;
  }
  CBFT_HIP(c->verdicts.reserve(((n + 63) / 64) * sizeof(uint64_t)));
  return CBFT_OK;
}

extern "C" {

const char* cbft_last_error(void) { return g_last_error; }

int cbft_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return CBFT_ENODEV;
  }
  return n;
}

const char* cbft_strerror(int code) {
  switch (code) {
    case CBFT_OK:
      return "ok";
    case CBFT_EINVAL:
      return "invalid argument";
    case CBFT_ENOMEM:
      return "out of memory";
    case CBFT_ENODEV:
      return "no such GPU / HIP runtime unavailable";
    case CBFT_EIO:
      return "HIP launch or copy failed";
    case CBFT_E2BIG:
      return "batch too large";
    default:
      return "unknown error";
  }
}

int cbft_open(cbft_ctx** out, int device, size_t max_batch) {
  if (!out) return CBFT_EINVAL;
  *out = nullptr;
  int ndev = cbft_device_count();
  if (ndev < 0) return ndev;
  if (device < 0 || device >= ndev) return CBFT_ENODEV;
  cbft_ctx* c = new (std::nothrow) cbft_ctx();
  if (!c) return CBFT_ENOMEM;
  c->device = device;
  int rc = CBFT_OK;
  do {
    if (hipSetDevice(device) != hipSuccess) {
      rc = CBFT_ENODEV;
      break;
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->compute[0], hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->compute[1], hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->build_stream, hipStreamNonBlocking) != hipSuccess) {
      rc = CBFT_EIO;
      break;
    }
    if (c->base_table.reserve(cbft_ed25519_base_table_words() * sizeof(uint32_t)) != hipSuccess) {
      rc = CBFT_ENOMEM;
      break;
    }
    if (cbft_ed25519_build_base_table(c->base_table.as<uint32_t>(), c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
      rc = CBFT_EIO;
      break;
    }
    if ((rc = build_base_comb(c)) != CBFT_OK) break;
    if (max_batch) rc = reserve_work(c, max_batch);
  } while (0);
  if (rc != CBFT_OK) {
    (void)hipGetLastError();
    cbft_close(c);
    return rc;
  }
  *out = c;
  return CBFT_OK;
}

int cbft_set_option(cbft_ctx* c, int option, int64_t v) {
  if (!c) return CBFT_EINVAL;
  if (!c->kids.empty()) {
    for (cbft_ctx* k : c->kids) {
      const int rc = cbft_set_option(k, option, v);
      if (rc) return rc;
    }
    return CBFT_OK;
  }
  std::lock_guard<std::mutex> g(c->mu);
  switch (option) {
    case CBFT_OPT_LADDER_LANES:
      if (v != 0 && v != 2 && v != 4) return CBFT_EINVAL;
      c->ladder_lanes = (int)v;
      return CBFT_OK;
    case CBFT_OPT_B_RADIX: {
      if (v < 16 || v > CBFT_COMB_MAX_RADIX) return CBFT_EINVAL;
      if (v == c->b_radix) return CBFT_OK;
      CBFT_HIP(hipSetDevice(c->device));
      CBFT_HIP(hipDeviceSynchronize());  // batches in flight read the old table
      c->base_comb.release();
      const int old = c->b_radix;
      c->b_radix = (int)v;
      const int rc = build_base_comb(c);
      if (rc) {  // back to the old radix (the context stays usable)
        c->b_radix = old;
        c->base_comb.release();
        (void)build_base_comb(c);
      }
      return rc;
    }
    case CBFT_OPT_WORK_SLOTS:
      if (v < 1 || v > CBFT_MAX_WORK_SLOTS) return CBFT_EINVAL;
      c->work_slots = (int)v;
      return CBFT_OK;
    case CBFT_OPT_SMALL_MAX:
      if (v < 0) return CBFT_EINVAL;
      c->small_max = (size_t)v;
      return CBFT_OK;
    case CBFT_OPT_SHA_SORT_MIN:
      if (v < 0) return CBFT_EINVAL;
      c->sha_sort_min = (size_t)v;
      return CBFT_OK;
    case CBFT_OPT_STAGE_ORDER:
      if (v < 0 || v > 2) return CBFT_EINVAL;
      c->stage_order = (int)v;
      return CBFT_OK;
    case CBFT_OPT_HASH_ORDER_EARLY:
      if (v < 0 || v > 1) return CBFT_EINVAL;
      c->hash_order_early = (int)v;
      return CBFT_OK;
    case CBFT_OPT_FINISH_K:
      if (v < 0 || v > 2) return CBFT_EINVAL;
      c->finish_k = (int)v;
      return CBFT_OK;
    default:
      return CBFT_EINVAL;
  }
}

int cbft_open_devices(cbft_ctx** out, const int* devices, int ndevices, size_t max_batch) {
  if (!out || !devices || ndevices < 1 || ndevices > 64) return CBFT_EINVAL;
  *out = nullptr;
  const int ndev = cbft_device_count();
  if (ndev < 0) return ndev;
  for (int i = 0; i < ndevices; i++)
    if (devices[i] < 0 || devices[i] >= ndev) return CBFT_ENODEV;
  if (ndevices == 1) return cbft_open(out, devices[0], max_batch);
  const std::vector<int> devs(devices, devices + ndevices);
  cbft_ctx* g = new (std::nothrow) cbft_ctx();
  if (!g) return CBFT_ENOMEM;
  g->device = devs[0];
  const size_t per = max_batch ? (max_batch + devs.size() - 1) / devs.size() + 64 : 0;
  for (int d : devs) {
    cbft_ctx* k = nullptr;
    const int rc = cbft_open(&k, d, per);
    if (rc) {
      cbft_close(g);
      return rc;
    }
    g->kids.push_back(k);
  }
  *out = g;
  return CBFT_OK;
}

int cbft_open_mask(cbft_ctx** out, uint32_t device_mask, size_t max_batch) {
  if (!out || !device_mask) return CBFT_EINVAL;
  int devs[32];
  int nd = 0;
  for (int d = 0; d < 32; d++)
    if ((device_mask >> d) & 1u) devs[nd++] = d;
  return cbft_open_devices(out, devs, nd, max_batch);
}

int cbft_device_of(cbft_ctx* c, int* out_devices, int max_out) {
  if (!c) return CBFT_EINVAL;
  const int n = c->kids.empty() ? 1 : (int)c->kids.size();
  for (int i = 0; i < n && i < max_out && out_devices; i++)
    out_devices[i] = c->kids.empty() ? c->device : c->kids[(size_t)i]->device;
  return n;
}

void cbft_close(cbft_ctx* c) {
  if (!c) return;
  if (!c->kids.empty()) {
    for (cbft_ctx* k : c->kids) cbft_close(k);
    delete c;
    return;
  }
  (void)hipSetDevice(c->device);
  for (HostSlot& hs : c->hslots) {
    std::lock_guard<std::mutex> g(hs.m);
    (void)collect_locked(hs);
  }
  for (hipStream_t st : {c->stream, c->copy_stream, c->compute[0], c->compute[1]})
    if (st) (void)hipStreamSynchronize(st);
  for (hipStream_t st : c->small_streams)
    if (st) (void)hipStreamSynchronize(st);
  if (c->build_stream) (void)hipStreamSynchronize(c->build_stream);
  for (auto& kv : c->tables) {
    std::lock_guard<std::mutex> ag(kv.second->append_mu);
    for (DevBuf& b : kv.second->chunks) b.release();
    kv.second->chunk_ptrs.release();
  }
  for (auto& kv : c->bls_sets) {
    kv.second.keys65.release();
    kv.second.lines.release();
    kv.second.ok.release();
    kv.second.aff.release();
  }
  for (DevBuf* b : {&c->bls_gen_lines, &c->bls_msg, &c->bls_H, &c->bls_shares, &c->bls_valid, &c->bls_sig,
                    &c->bls_ids, &c->bls_use, &c->bls_lambda, &c->bls_partial, &c->bls_out,
                    &c->bls_ms_ok, &c->bls_bitmap, &c->bls_inv, &c->bls_first, &c->bls_flag, &c->bls_g2tmp,
                    &c->bls_pub_tbl})
    b->release();
  (void)hipDeviceSynchronize();  // device-path batches may still run on caller streams
  for (DevBuf* b : {&c->base_table, &c->base_comb, &c->verdicts, &c->sig, &c->msg, &c->off, &c->len, &c->kidx, &c->pk,
                    &c->dstage})
    b->release();
  c->hstage.release();
  for (WorkSlot& w : c->slots) {
    for (DevBuf* b : {&w.h, &w.flags, &w.xyz, &w.ps_tbl, &w.ps_aok, &w.perm, &w.buckets}) b->release();
    if (w.done) (void)hipEventDestroy(w.done);
    if (w.fork) (void)hipEventDestroy(w.fork);
    if (w.join) (void)hipEventDestroy(w.join);
    if (w.aux) (void)hipStreamDestroy(w.aux);
  }
  for (hipEvent_t& e : c->ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t& e : c->stage_done)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ring)
    if (e) (void)hipEventDestroy(e);
  cbft_sign_release(c);
  cbft_rsa_sign_release(c);
  cbft_bls_sign_release(c);
  cbft_bls_verify_batch_release(c);
  cbft_bls_combine_batch_release(c);
  cbft_bls_multisig_batch_release(c);
  cbft_bls_keygen_release(c);
  cbft_ecdsa_release(c);
  cbft_ecdsa_sign_release(c);
  for (auto& kv : c->rsa_tables) kv.second.rec.release();
  for (DevBuf* b : {&c->rsav.sig, &c->rsav.kidx}) b->release();
  c->rsav.scratch.release();
  c->rsav.timer.release();
  for (HostSlot& hs : c->hslots) {
    for (DevBuf* b : {&hs.in, &hs.verd}) b->release();
    hs.pack.release();
    hs.hverd.release();
    for (hipEvent_t e : {hs.copied, hs.done, hs.done_blk})
      if (e) (void)hipEventDestroy(e);
  }
  for (hipStream_t st : {c->stream, c->copy_stream, c->compute[0], c->compute[1], c->build_stream})
    if (st) (void)hipStreamDestroy(st);
  for (hipStream_t st : c->small_streams)
    if (st) (void)hipStreamDestroy(st);
  delete c;
}

int cbft_set_profiling(cbft_ctx* c, int enable) {
  c = cbft_dev0(c);
  if (!c) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  if (enable < 0 || enable > 2) return CBFT_EINVAL;
  if (enable && !c->ev[0])
    for (hipEvent_t& e : c->ev) CBFT_HIP(hipEventCreate(&e));
  if (enable == 2 && c->ring.empty()) {
    c->ring.assign(CBFT_PROF_RING * 4, nullptr);
    for (hipEvent_t& e : c->ring) CBFT_HIP(hipEventCreate(&e));
  }
  c->profiling = enable != 0;
  c->prof_mode = enable;
  c->ring_n = 0;
  c->ev_valid = false;
  return CBFT_OK;
}

int cbft_stage_times_avg_ms(cbft_ctx* c, float* out, int nout, int* nbatches) {
  c = cbft_dev0(c);
  if (!c || !out || nout < 3) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  if (c->prof_mode != 2 || c->ring_n == 0) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  const size_t cnt = std::min<size_t>(c->ring_n, CBFT_PROF_RING);
  double sum[3] = {0, 0, 0};
  for (size_t b = 0; b < cnt; b++) {
    hipEvent_t* e = &c->ring[b * 4];
    CBFT_HIP(hipEventSynchronize(e[3]));
    for (int k = 0; k < 3; k++) {
      float ms = 0;
      CBFT_HIP(hipEventElapsedTime(&ms, e[k], e[k + 1]));
      sum[k] += ms;
    }
  }
  for (int k = 0; k < 3; k++) out[k] = (float)(sum[k] / (double)cnt);
  if (nbatches) *nbatches = (int)cnt;
  return CBFT_OK;
}

int cbft_stage_times_ms(cbft_ctx* c, float* out, int nout) {
  c = cbft_dev0(c);
  if (!c || !out || nout < 3) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->ev_valid) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(hipEventSynchronize(c->ev[3]));
  for (int k = 0; k < 3; k++) CBFT_HIP(hipEventElapsedTime(&out[k], c->ev[k], c->ev[k + 1]));
  return CBFT_OK;
}

int cbft_sync(cbft_ctx* c) {
  if (!c) return CBFT_EINVAL;
  for (cbft_ctx* k : c->kids) {
    const int rc = cbft_sync(k);
    if (rc) return rc;
  }
  if (!c->kids.empty()) return CBFT_OK;
  (void)hipSetDevice(c->device);
  for (hipStream_t st : {c->stream, c->copy_stream, c->compute[0], c->compute[1]}) CBFT_HIP(hipStreamSynchronize(st));
  for (hipStream_t st : c->small_streams)
    if (st) CBFT_HIP(hipStreamSynchronize(st));
  return CBFT_OK;
}

static int append_keys(cbft_ctx* c, uint32_t id, const uint8_t* pk, uint32_t nkeys, uint32_t* out_first,
                       bool check_budget);

// Load a key table on one device under `id` (a multi-device context's parent picks the id, so
// every device holds the table under the same id), or under the device's next id when id == 0.
static int load_keys_on(cbft_ctx* c, const uint8_t* pk, uint32_t nkeys, int comb_radix, uint32_t want_id,
                        uint32_t* out_id) {
  CBFT_HIP(hipSetDevice(c->device));
  auto kt = std::make_shared<KeyTable>();
  kt->geo = cbft_comb_geom(key_radix(comb_radix, nkeys));
  CBFT_HIP(kt->chunk_ptrs.reserve(CBFT_MAX_KEY_CHUNKS * sizeof(void*)));
  uint32_t id = want_id;
  {
    std::lock_guard<std::mutex> g(c->mu);
    if (!id) {
      id = c->next_table_id++;
      if (id == CBFT_NO_KEY_TABLE) id = c->next_table_id++;
    }
    if (!c->tables.emplace(id, kt).second) return CBFT_EIO;
  }
  if (nkeys) {
    uint32_t first = 0;
    const int rc = append_keys(c, id, pk, nkeys, &first, comb_radix == 0);
    if (rc) {
      (void)cbft_ed25519_unload_keys(c, id);
      return rc;
    }
  }
  *out_id = id;
  return CBFT_OK;
}

int cbft_ed25519_load_keys_ex(cbft_ctx* c, const uint8_t* pk, uint32_t nkeys, int comb_radix, uint32_t* out_id) {
  if (!c || !out_id || (nkeys && !pk)) return CBFT_EINVAL;
  if (comb_radix && (comb_radix < 8 || comb_radix > 15)) return CBFT_EINVAL;
  if (c->kids.empty()) return load_keys_on(c, pk, nkeys, comb_radix, 0, out_id);
  // replicate the table on every device, concurrently, under one id the parent allocates; if any
  // device fails, the devices that loaded it unload it again (no device keeps a table the others
  // lack, and the ids stay in step for every later load)
  uint32_t id;
  {
    std::lock_guard<std::mutex> g(c->mu);
    id = c->next_table_id++;
    if (id == CBFT_NO_KEY_TABLE) id = c->next_table_id++;
  }
  std::vector<int> rcs(c->kids.size(), CBFT_OK);
  (void)for_each_kid(c, [&](size_t g) {
    uint32_t got = 0;
    return rcs[g] = load_keys_on(c->kids[g], pk, nkeys, comb_radix, id, &got);
  });
  int rc = CBFT_OK;
  for (int r : rcs)
    if (r && !rc) rc = r;
  if (rc) {
    for (size_t g = 0; g < c->kids.size(); g++)
      if (rcs[g] == CBFT_OK) (void)cbft_ed25519_unload_keys(c->kids[g], id);
    return rc;
  }
  *out_id = id;
  return CBFT_OK;
}

int cbft_ed25519_load_keys(cbft_ctx* c, const uint8_t* pk, uint32_t nkeys, uint32_t* out_id) {
  return cbft_ed25519_load_keys_ex(c, pk, nkeys, 0, out_id);
}

static std::shared_ptr<KeyTable> find_table(cbft_ctx* c, uint32_t id) {
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->tables.find(id);
  return it == c->tables.end() ? nullptr : it->second;
}

// HBM budget of one key table's comb tables ($CBFT_COMB_BUDGET_GB, default 64 GB of 288 GB).
static double comb_budget_bytes() {
  double budget = 64.0;
  if (const char* e = getenv("CBFT_COMB_BUDGET_GB")) budget = atof(e);
  return budget * 1e9;
}

// Write keys [k0, k0 + n) of a table (their raw encodings from pk, host or device memory): new
// chunks as needed (their pointers appended to the device chunk array), then on the build stream
// one staging copy of the n keys, ONE position-point launch for all of them (decode verdicts,
// 2^(w j) (-A)), the raw keys and verdicts into their chunk slots, and the table lanes in
// launches that span chunks (through the device chunk-pointer array); one synchronisation at
// the end, staging allocated once per call.
static int fill_keys(cbft_ctx* c, KeyTable& kt, const uint8_t* pk, hipMemcpyKind kind, uint32_t k0, uint32_t n) {
  const size_t wpk = kt.geo.words_per_unit();
  hipStream_t s = c->build_stream;
  while (kt.chunks.size() * CBFT_KEY_CHUNK < (size_t)k0 + n) {
    DevBuf b;
    CBFT_HIP(b.reserve(cbft_key_chunk_bytes(wpk)));
    const size_t ci = kt.chunks.size();
    kt.chunks.push_back(b);
    CBFT_HIP(hipMemcpyAsync(kt.chunk_ptrs.as<void*>() + ci, &kt.chunks.back().p, sizeof(void*),
                            hipMemcpyHostToDevice, s));
    CBFT_HIP(hipStreamSynchronize(s));  // the source is a host variable
  }
  if (n == 0) return CBFT_OK;
  const size_t lanes = (size_t)n * kt.geo.npos * kt.geo.chunks();
  const size_t step = std::min(lanes, kCombBuildLanes);
  DevBuf raw, pos, aok, tmp;
  hipError_t e = raw.reserve((size_t)n * 32);
  if (e == hipSuccess) e = pos.reserve(cbft_ed25519_comb_pos_words(n, kt.geo) * sizeof(uint32_t));
  if (e == hipSuccess) e = aok.reserve(n);
  if (e == hipSuccess) e = tmp.reserve(cbft_ed25519_comb_tmp_words(step) * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpyAsync(raw.p, pk, (size_t)n * 32, kind, s);
  if (e == hipSuccess)
    e = cbft_ed25519_launch_comb_pos(raw.as<uint8_t>(), n, 1, kt.geo, pos.as<uint32_t>(), aok.as<uint8_t>(), s);
  for (uint32_t a = k0; e == hipSuccess && a < k0 + n;) {  // raw keys and verdicts into the chunk slots
    const uint32_t ci = a >> CBFT_KEY_CHUNK_SHIFT, slot = a & (CBFT_KEY_CHUNK - 1);
    const uint32_t m = std::min<uint32_t>(k0 + n - a, CBFT_KEY_CHUNK - slot);
    uint8_t* base = kt.chunks[ci].as<uint8_t>();
    uint8_t* dpk = base + (size_t)CBFT_KEY_CHUNK * wpk * 4 + (size_t)slot * 32;
    uint8_t* daok = base + (size_t)CBFT_KEY_CHUNK * (wpk * 4 + 32) + slot;
    e = hipMemcpyAsync(dpk, raw.as<uint8_t>() + (size_t)(a - k0) * 32, (size_t)m * 32, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(daok, aok.as<uint8_t>() + (a - k0), m, hipMemcpyDeviceToDevice, s);
    a += m;
  }
  for (size_t l0 = 0; e == hipSuccess && l0 < lanes; l0 += step)  // table lanes across chunks
    e = cbft_ed25519_launch_comb_tables(pos.as<uint32_t>(), n, kt.geo, nullptr, kt.chunk_ptrs.as<void*>(), k0,
                                        tmp.as<uint32_t>(), l0, std::min(step, lanes - l0), s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  raw.release();
  pos.release();
  aok.release();
  tmp.release();
  if (e != hipSuccess) return cbft_fail(e, "comb table build", __FILE__, __LINE__);
  return CBFT_OK;
}

// Raw key encodings [0, nkeys) of a table, device to device, as the source of a rebuild.
static const uint8_t* chunk_raw_keys(const KeyTable& kt, uint32_t ci) {
  return kt.chunks[ci].as<uint8_t>() + (size_t)CBFT_KEY_CHUNK * kt.geo.words_per_unit() * 4;
}

// Append keys to a table — verifies of the published keys continue meanwhile: everything is
// built outside the context mutex, then the new key count is published.  Appends to one table
// are serialised by its append_mu.  When the grown table would exceed the HBM budget at its comb
// radix, the whole table is rebuilt at the widest radix that fits (13 -> 11 -> 8; the published
// keys' raw encodings are copied device to device) and swapped in under the mutex; batches
// already queued against the old table finish before it is released.  Past the budget at radix
// 8 the append fails with CBFT_ENOMEM and the table is unchanged.
int cbft_ed25519_append_keys(cbft_ctx* c, uint32_t id, const uint8_t* pk, uint32_t nkeys, uint32_t* out_first) {
  return append_keys(c, id, pk, nkeys, out_first, true);
}

// check_budget = false: the initial fill of a table whose radix the caller chose explicitly
// (cbft_ed25519_load_keys_ex with comb_radix != 0) is built at that radix whatever the budget.
static int append_keys(cbft_ctx* c, uint32_t id, const uint8_t* pk, uint32_t nkeys, uint32_t* out_first,
                       bool check_budget) {
  if (!c || !out_first || (nkeys && !pk)) return CBFT_EINVAL;
  if (!c->kids.empty()) {  // every device concurrently
    std::vector<uint32_t> firsts(c->kids.size(), 0);
    const int rc = for_each_kid(c, [&](size_t g) {
      return append_keys(c->kids[g], id, pk, nkeys, &firsts[g], check_budget);
    });
    if (rc) return rc;
    for (uint32_t f : firsts)
      if (f != firsts[0]) return CBFT_EIO;
    *out_first = firsts[0];
    return CBFT_OK;
  }
  std::shared_ptr<KeyTable> kt;
  std::unique_lock<std::mutex> ag;
  for (;;) {  // a concurrent re-radix may replace the table while we wait for its append_mu
    kt = find_table(c, id);
    if (!kt) return CBFT_EINVAL;
    ag = std::unique_lock<std::mutex>(kt->append_mu);
    if (find_table(c, id) == kt) break;
    ag.unlock();
  }
  CBFT_HIP(hipSetDevice(c->device));
  uint32_t k0;
  {
    std::lock_guard<std::mutex> g(c->mu);
    k0 = kt->nkeys;
  }
  *out_first = k0;
  if (!nkeys) return CBFT_OK;
  if ((uint64_t)k0 + nkeys > (uint64_t)CBFT_MAX_KEY_CHUNKS * CBFT_KEY_CHUNK) return CBFT_E2BIG;
  const uint32_t total = k0 + nkeys;
  const double budget = comb_budget_bytes();
  auto fits = [&](int r) { return table_bytes(total, r) <= budget; };
  if (!check_budget || fits(kt->geo.w)) {
    const int rc = fill_keys(c, *kt, pk, hipMemcpyHostToDevice, k0, nkeys);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    kt->nkeys = total;
    return CBFT_OK;
  }
  int r2 = 0;
  for (int r : {13, 11, 8})
    if (r < kt->geo.w && fits(r)) {
      r2 = r;
      break;
    }
  if (!r2) return CBFT_ENOMEM;
  // A rebuild holds the old and the new table at once (plus the build staging) until the swap:
  // refuse it up front, table unchanged, when the device cannot hold the new one beside the old.
  {
    size_t free_b = 0, total_b = 0;
    CBFT_HIP(hipMemGetInfo(&free_b, &total_b));
    const double staging = (double)cbft_ed25519_comb_tmp_words(kCombBuildLanes) * 4.0;
    if (table_bytes(total, r2) + staging > (double)free_b) return CBFT_ENOMEM;
  }
  auto nt = std::make_shared<KeyTable>();
  nt->geo = cbft_comb_geom(r2);
  CBFT_HIP(nt->chunk_ptrs.reserve(CBFT_MAX_KEY_CHUNKS * sizeof(void*)));
  int rc = CBFT_OK;
  for (uint32_t ci = 0; rc == CBFT_OK && (size_t)ci * CBFT_KEY_CHUNK < k0; ci++)
    rc = fill_keys(c, *nt, chunk_raw_keys(*kt, ci), hipMemcpyDeviceToDevice, ci * CBFT_KEY_CHUNK,
                   std::min<uint32_t>(CBFT_KEY_CHUNK, k0 - ci * CBFT_KEY_CHUNK));
  if (rc == CBFT_OK) rc = fill_keys(c, *nt, pk, hipMemcpyHostToDevice, k0, nkeys);
  if (rc) {
    for (DevBuf& b : nt->chunks) b.release();
    nt->chunk_ptrs.release();
    return rc;
  }
  {
    std::lock_guard<std::mutex> g(c->mu);
    nt->nkeys = total;
    c->tables[id] = nt;  // new batches use the rebuilt table from here on
  }
  (void)hipDeviceSynchronize();  // batches queued against the old table (any stream) finish
  for (DevBuf& b : kt->chunks) b.release();
  kt->chunk_ptrs.release();
  return CBFT_OK;
}

// Rebuild key slots in place with new keys (a rotated key reusing a released slot).  The caller
// guarantees no batch in flight names these slots; the device is synchronised first anyway.
int cbft_ed25519_replace_keys(cbft_ctx* c, uint32_t id, const uint32_t* idx, const uint8_t* pk, uint32_t n) {
  if (!c || (n && (!idx || !pk))) return CBFT_EINVAL;
  if (!c->kids.empty()) {
    for (cbft_ctx* k : c->kids) {
      const int rc = cbft_ed25519_replace_keys(k, id, idx, pk, n);
      if (rc) return rc;
    }
    return CBFT_OK;
  }
  std::shared_ptr<KeyTable> kt;
  std::unique_lock<std::mutex> ag;
  for (;;) {
    kt = find_table(c, id);
    if (!kt) return CBFT_EINVAL;
    ag = std::unique_lock<std::mutex>(kt->append_mu);
    if (find_table(c, id) == kt) break;
    ag.unlock();
  }
  uint32_t have;
  {
    std::lock_guard<std::mutex> g(c->mu);
    have = kt->nkeys;
  }
  for (uint32_t i = 0; i < n; i++)
    if (idx[i] >= have) return CBFT_EINVAL;
  CBFT_HIP(hipSetDevice(c->device));
  CBFT_HIP(hipDeviceSynchronize());
  for (uint32_t i = 0; i < n; i++) {
    const int rc = fill_keys(c, *kt, pk + (size_t)i * 32, hipMemcpyHostToDevice, idx[i], 1);
    if (rc) return rc;
  }
  return CBFT_OK;
}

int cbft_ed25519_table_size(cbft_ctx* c, uint32_t id, uint32_t* out_nkeys, int* out_radix) {
  if (!c || !out_nkeys) return CBFT_EINVAL;
  auto kt = find_table(cbft_dev0(c), id);
  if (!kt) return CBFT_EINVAL;
  std::lock_guard<std::mutex> g(cbft_dev0(c)->mu);
  *out_nkeys = kt->nkeys;
  if (out_radix) *out_radix = kt->geo.w;
  return CBFT_OK;
}

int cbft_ed25519_unload_keys(cbft_ctx* c, uint32_t id) {
  if (!c) return CBFT_EINVAL;
  if (!c->kids.empty()) {
    int rc = CBFT_OK;
    for (cbft_ctx* k : c->kids) {
      const int r = cbft_ed25519_unload_keys(k, id);
      if (r && !rc) rc = r;
    }
    return rc;
  }
  std::shared_ptr<KeyTable> kt;
  {
    std::lock_guard<std::mutex> g(c->mu);
    auto it = c->tables.find(id);
    if (it == c->tables.end()) return CBFT_EINVAL;
    kt = it->second;
    c->tables.erase(it);  // no new batch can name it
  }
  std::lock_guard<std::mutex> ag(kt->append_mu);  // an append in progress finishes first
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();  // in-flight batches (any stream) read it
  for (DevBuf& b : kt->chunks) b.release();
  kt->chunk_ptrs.release();
  return CBFT_OK;
}

// Launch the verify pipeline for a batch whose inputs are already on the device.
// uniform_blocks: the caller knows every message has the same SHA-512 block count (no sort)
static int launch_locked(cbft_ctx* c, uint32_t table_id, const uint8_t* d_pk, const uint32_t* d_kidx,
                         const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_off, const uint32_t* d_len,
                         uint32_t fixed_len, size_t n, uint64_t* d_verdicts, hipStream_t s,
                         bool uniform_blocks = false) {
  int rc = reserve_work(c, n);
  if (rc) return rc;
  KeyTable* kt = nullptr;
  if (table_id != CBFT_NO_KEY_TABLE) {
    auto it = c->tables.find(table_id);
    if (it == c->tables.end() || !d_kidx) return CBFT_EINVAL;
    kt = it->second.get();
  }
  // the fused small-batch kernel keeps everything in registers: no work slot to order against
  const bool small = kt && n <= c->small_max && !c->ladder_lanes;
  WorkSlot& slot = c->slots[small ? 0 : c->next_slot++ % (unsigned)c->work_slots];
  if (!small) {
    if (table_id == CBFT_NO_KEY_TABLE) {
      CBFT_HIP(slot.ps_tbl.reserve(n * cbft_ed25519_table_words_per_unit() * sizeof(uint32_t)));
      CBFT_HIP(slot.ps_aok.reserve(n));
    }
    // the slot's previous batch (maybe on another stream) must be done with its buffers
    if (slot.used) CBFT_HIP(hipStreamWaitEvent(s, slot.done, 0));
  }
  // variable-length batches from sha_sort_min signatures (default 4,096; 0 = never) hash
  // in order of their SHA-512 block count (SURVEY.md §7 hard part ii)
  const bool sort = !small && d_off && !uniform_blocks && c->sha_sort_min && n >= c->sha_sort_min;
  if (sort) {
    CBFT_HIP(slot.perm.reserve(n * sizeof(uint32_t)));
    if (!slot.buckets.p) {  // counts | cursors | uniform flag | n_short
      CBFT_HIP(slot.buckets.reserve((2 * CBFT_SHA_BUCKETS + 2) * sizeof(uint32_t)));
      CBFT_HIP(hipMemsetAsync(slot.buckets.p, 0, (2 * CBFT_SHA_BUCKETS + 2) * sizeof(uint32_t), s));  // counts start at 0
    }
    if (!slot.aux) {  // the long-message hash stream
      CBFT_HIP(hipStreamCreateWithFlags(&slot.aux, hipStreamNonBlocking));
      CBFT_HIP(hipEventCreateWithFlags(&slot.fork, hipEventDisableTiming));
      CBFT_HIP(hipEventCreateWithFlags(&slot.join, hipEventDisableTiming));
    }
  }

  Ed25519Batch b{n, d_pk, d_kidx, KeyChunks{nullptr, 0}, d_sig, d_msg, d_off, d_len,
                 kt ? kt->nkeys : (uint32_t)n, fixed_len};
  Ed25519Work w{};
  // one inversion per finish block of 64 lanes x finish_k signatures (the tree finish, its root
  // inverted on the scalar unit): 2 per lane from 16K signatures (512 blocks at 64K), else 1
  w.finish_k = c->finish_k ? c->finish_k : (n >= 16384 ? 2 : 1);
  w.base_table = c->base_table.as<uint32_t>();
  w.h_soa = slot.h.as<uint32_t>();
  w.flags = slot.flags.as<uint8_t>();
  w.xyz_soa = slot.xyz.as<uint32_t>();
  w.verdict_words = d_verdicts;
  if (sort) {
    w.perm = slot.perm.as<uint32_t>();
    w.buckets = slot.buckets.as<uint32_t>();
    w.aux = slot.aux;
    w.fork_ev = slot.fork;
    w.join_ev = slot.join;
  }
  if (table_id == CBFT_NO_KEY_TABLE) {
    // per-signature keys: decode + precompute per signature
    CBFT_HIP(cbft_ed25519_launch_prep(d_pk, n, slot.ps_tbl.as<uint32_t>(), slot.ps_aok.as<uint8_t>(), s));
    b.key_idx = nullptr;
    w.tbl = slot.ps_tbl.as<uint32_t>();
    w.aok = slot.ps_aok.as<uint8_t>();
  } else {
    b.pk = nullptr;
    b.keys = kt->view();
    w.base_comb = c->base_comb.as<uint32_t>();
    w.comb = cbft_comb_ladder(kt->geo.w, c->b_radix);
    // pair ladder (fewer additions in total, 2 waves/SIMD) once a batch fills the chip with it;
    // the quad ladder (half the additions per lane) for the latency of small batches
    w.comb_lanes = c->ladder_lanes ? c->ladder_lanes : (n >= 32768 ? 2 : 4);
    w.small = small ? 1 : 0;
  }
  // Stage order pays for big batches (their stages fill the chip; see cbft_ctx::stage_order).
  // Small batches are latency-bound single waves per stage: ordering them only serialises
  // concurrent callers' batches (the per-request coalescer keeps several in flight), so they run
  // unordered (from 4,096 signatures).
  const int so = sort ? c->stage_order_var : c->stage_order;
  bool ordered = so && n >= c->stage_order_min && !w.small;
  if (ordered) {  // how many streams do the recent big batches use?
    c->recent_streams[c->recent_n++ % 4] = s;
    unsigned distinct = 0;
    for (unsigned a = 0; a < 4 && a < c->recent_n; a++) {
      bool seen = false;
      for (unsigned q = 0; q < a; q++) seen = seen || c->recent_streams[q] == c->recent_streams[a];
      distinct += seen ? 0u : 1u;
    }
    if ((int)distinct > c->order_max_streams) ordered = false;
  }
  StageOrder order{};
  if (ordered) {
    for (hipEvent_t& e : c->stage_done)
      if (!e) CBFT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    order.wait = c->stage_used;
    order.hash = so != 2;  // 2: ladders only
    order.ladder = true;
    order.done[0] = c->stage_done[0];
    order.done[1] = c->stage_done[1];
    order.hash_early = c->hash_order_early != 0;
  }
  hipEvent_t* evp = nullptr;
  if (c->profiling) evp = c->prof_mode == 2 ? &c->ring[(c->ring_n++ % CBFT_PROF_RING) * 4] : c->ev;
  CBFT_HIP(cbft_ed25519_launch_verify(b, w, s, evp, ordered ? &order : nullptr));
  if (ordered) c->stage_used = true;
  if (!small) {
    CBFT_HIP(hipEventRecord(slot.done, s));
    slot.used = true;
  }
  c->ev_valid = c->profiling;
  return CBFT_OK;
}

// ---------------------------------------------------------------- pinned host memory
// Registry of cbft_host_alloc blocks (process-wide, so a multi-GPU context's children see the
// blocks allocated through the group).  Host-buffer entry points DMA any input that lies inside
// one of them straight to the device; other inputs are packed into a pinned image first.
static std::mutex g_pin_mu;
static std::map<uintptr_t, size_t> g_pinned;  // base -> bytes

static bool is_pinned(const void* p, size_t bytes) {
  if (!p || !bytes) return false;
  std::lock_guard<std::mutex> g(g_pin_mu);
  auto it = g_pinned.upper_bound((uintptr_t)p);
  if (it == g_pinned.begin()) return false;
  --it;
  return (uintptr_t)p + bytes <= it->first + it->second;
}

static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

#define CBFT_PACK_MAX (4u << 20)  // pageable bytes of one batch packed into pinned staging

// Device image of one host-buffer batch: [key idx | keys][sig][off][len][messages], 256-B aligned
// parts (no off/len for fixed-length batches).
struct BatchLayout {
  size_t key, sig, off, len, msg;
};
static void batch_layout(size_t n, bool key_table, bool fixed, BatchLayout& l) {
  l.key = 0;
  l.sig = up256(l.key + (key_table ? n * 4 : n * 32));
  l.off = up256(l.sig + n * 64);
  l.len = up256(l.off + (fixed ? 0 : n * 8));
  l.msg = up256(l.len + (fixed ? 0 : n * 4));
}

// Deliver a slot's verdicts to its batch's bitmap, waiting for the batch.  Caller holds s.m.
static int collect_locked(HostSlot& s) {
  if (!s.pending) return s.status;
  s.pending = false;
  hipError_t e = hipEventSynchronize(s.wait_ev ? s.wait_ev : s.done);
  if (e != hipSuccess) return s.status = cbft_fail(e, "hipEventSynchronize(batch done)", __FILE__, __LINE__);
  const size_t nbytes = (s.n + 7) / 8;
  std::memcpy(s.bitmap, s.hverd.p, nbytes);  // little-endian host: verdict words == bitmap bytes
  if (s.n % 8) s.bitmap[nbytes - 1] &= (uint8_t)((1u << (s.n % 8)) - 1);
  return s.status = CBFT_OK;
}

// Queue one host-buffer batch: H2D on the copy stream (pinned inputs DMA'd directly, pageable
// ones packed into the slot's pinned image and moved with one DMA), the verify pipeline on one of
// the two compute streams after the copy, the verdict words D2H into pinned memory.  Returns
// once queued; cbft_wait (or a later submission that needs the slot) delivers the bitmap.
// fixed_len: msg_off/msg_len are unused, message i = msg_blob[i * fixed_len, ...).
static int submit_host(cbft_ctx* c, uint32_t table_id, const uint8_t* pk, const uint32_t* key_idx, const uint8_t* sig,
                       const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len, bool fixed,
                       uint32_t fixed_len, size_t n, uint8_t* bitmap, uint64_t* ticket) {
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  const bool kt = table_id != CBFT_NO_KEY_TABLE;
  uint32_t nkeys = 0;
  if (kt) {
    auto it = c->tables.find(table_id);
    if (it == c->tables.end() || !key_idx) return CBFT_EINVAL;
    nkeys = it->second->nkeys;
    for (size_t i = 0; i < n; i++)
      if (key_idx[i] >= nkeys) return CBFT_EINVAL;
  } else if (!pk) {
    return CBFT_EINVAL;
  }
  // message bytes to move: [blo, bhi) of the blob (offsets need not start at 0)
  uint64_t blo = 0, bhi = 0;
  uint32_t lmin = 0, lmax = 0;  // message lengths: one SHA-512 block count for all -> no hash sort
  bool packed = !fixed && n;    // message i at msg_off[0] + i * msg_len[0], one length for all
  if (fixed) {
    bhi = (uint64_t)fixed_len * n;
  } else if (n) {
    blo = msg_off[0];
    lmin = UINT32_MAX;
    for (size_t i = 0; i < n; i++) {
      blo = std::min<uint64_t>(blo, msg_off[i]);
      bhi = std::max<uint64_t>(bhi, msg_off[i] + msg_len[i]);
      lmin = std::min(lmin, msg_len[i]);
      lmax = std::max(lmax, msg_len[i]);
      packed = packed && msg_len[i] == msg_len[0] && msg_off[i] == msg_off[0] + (uint64_t)i * msg_len[0];
    }
  }
  const bool uniform_blocks = (64u + (uint64_t)lmin + 17u + 127u) / 128u == (64u + (uint64_t)lmax + 17u + 127u) / 128u;
  // Same-length messages laid end to end (a packed blob: SigManager's batches of equal-size
  // requests, the per-request engine's coalesced calls of one size) run as a fixed-length batch:
  // no offset / length arrays to move, and the kernels read message i at i * len directly (no
  // dependent offset read, which on the zero-copy path is a PCIe round trip)
  if (packed) {
    fixed = true;
    fixed_len = msg_len[0];
    blo = msg_off[0];
    bhi = blo + (uint64_t)fixed_len * n;
  }
  const uint64_t mbase = fixed ? 0 : blo;  // message addresses in the image: o_msg + (off - mbase)
  const uint64_t blob = bhi - blo;
  if (blob && !msg_blob) return CBFT_EINVAL;
  int rc = reserve_work(c, n);
  if (rc) return rc;
  const uint64_t t = ++c->next_ticket;
  HostSlot& s = c->hslots[t % CBFT_HOST_SLOTS];
  std::lock_guard<std::mutex> sg(s.m);
  rc = collect_locked(s);  // the slot's previous batch, if nobody has waited for it yet
  if (rc) return rc;
  const size_t nw = (n + 63) / 64;
  BatchLayout lay;
  batch_layout(n, kt, fixed, lay);
  const size_t o_key = lay.key, o_sig = lay.sig, o_off = lay.off, o_len = lay.len, o_msg = lay.msg;
  const size_t in_bytes = o_msg + blob + 16;
  CBFT_HIP(s.in.reserve(in_bytes));
  CBFT_HIP(s.verd.reserve(nw * 8));
  CBFT_HIP(s.hverd.reserve(nw * 8));
  if (!s.copied) CBFT_HIP(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
  if (!s.done) CBFT_HIP(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  if (!s.done_blk) CBFT_HIP(hipEventCreateWithFlags(&s.done_blk, hipEventDisableTiming | hipEventBlockingSync));
  s.wait_ev = s.done;
  struct Part {
    const void* src;
    size_t bytes, off;
  } parts[5] = {{kt ? static_cast<const void*>(key_idx) : static_cast<const void*>(pk), kt ? n * 4 : n * 32, o_key},
                {sig, n * 64, o_sig},
                {msg_off, fixed ? 0 : n * 8, o_off},
                {msg_len, fixed ? 0 : n * 4, o_len},
                {msg_blob ? msg_blob + blo : nullptr, (size_t)blob, o_msg}};
  // pinned[k]: DMA straight from the caller's block.  Pageable parts of a small batch (total <=
  // CBFT_PACK_MAX bytes: the latency path, p50 @ 1K) are packed into the slot's pinned image and
  // moved by one DMA; larger pageable parts go through the runtime's own pipelined staging
  // (hipMemcpyAsync from pageable memory), which beats a serial host memcpy into pinned memory.
  bool pinned[5];
  size_t pageable = 0;
  for (int k = 0; k < 5; k++) {
    pinned[k] = is_pinned(parts[k].src, parts[k].bytes);
    if (parts[k].bytes && !pinned[k]) pageable += parts[k].bytes;
  }
  const bool pack = pageable <= CBFT_PACK_MAX;
  size_t plo = SIZE_MAX, phi = 0;
  for (int k = 0; k < 5; k++)
    if (parts[k].bytes && !pinned[k] && pack) {
      plo = std::min(plo, parts[k].off);
      phi = std::max(phi, parts[k].off + parts[k].bytes);
    }
  uint8_t* din = s.in.as<uint8_t>();
  // a small packed batch (the per-request path) copies on its compute stream: no copy-stream
  // event to record and wait for; bigger batches overlap their copies with earlier batches' kernels
  const bool one_stream = pack && n <= c->small_max;
  hipStream_t cs = c->compute[t & 1];
  if (one_stream) {
    hipStream_t& ss = c->small_streams[t % CBFT_SMALL_STREAMS];
    if (!ss) CBFT_HIP(hipStreamCreateWithFlags(&ss, hipStreamNonBlocking));
    cs = ss;
  }
  hipStream_t cps = one_stream ? cs : c->copy_stream;
  // zero-copy: a fused small batch whose parts are all pageable (the per-request coalescer's
  // case) is packed into the slot's pinned image and the kernel reads it there over PCIe and
  // writes its verdict words straight into pinned memory: one launch and one event per batch
  // instead of two DMAs around the launch (the host API time of the copies bounded the
  // coalescer's batch rate)
  bool zc = one_stream && kt && !c->ladder_lanes;
  for (int k = 0; k < 5 && zc; k++)
    if (parts[k].bytes && pinned[k]) zc = false;
  if (zc) {
    CBFT_HIP(s.pack.reserve(in_bytes));
    for (int k = 0; k < 5; k++)
      if (parts[k].bytes) std::memcpy(s.pack.as<uint8_t>(parts[k].off), parts[k].src, parts[k].bytes);
    const uint8_t* zin = static_cast<const uint8_t*>(s.pack.dev);
    rc = launch_locked(c, table_id, nullptr, reinterpret_cast<const uint32_t*>(zin + o_key), zin + o_sig,
                       zin + o_msg - mbase, fixed ? nullptr : reinterpret_cast<const uint64_t*>(zin + o_off),
                       fixed ? nullptr : reinterpret_cast<const uint32_t*>(zin + o_len), fixed_len, n,
                       static_cast<uint64_t*>(s.hverd.dev), cs, uniform_blocks);
    if (rc) return rc;
    s.wait_ev = s.done_blk;
    CBFT_HIP(hipEventRecord(s.wait_ev, cs));
    s.ticket = t;
    s.pending = true;
    s.status = CBFT_OK;
    s.n = n;
    s.bitmap = bitmap;
    *ticket = t;
    return CBFT_OK;
  }
  // every part pinned and laid out in one host block exactly as in the device image
  // (cbft_ed25519_batch_layout): the whole batch is one DMA
  {
    const uint8_t* base = nullptr;
    size_t lo = SIZE_MAX, hi = 0;
    bool same = true;
    for (int k = 0; k < 5 && same; k++) {
      if (!parts[k].bytes) continue;
      const uint8_t* src = static_cast<const uint8_t*>(parts[k].src);
      if (!pinned[k]) same = false;
      else if (!base) base = src - parts[k].off;
      else if (src - parts[k].off != base) same = false;
      lo = std::min(lo, parts[k].off);
      hi = std::max(hi, parts[k].off + parts[k].bytes);
    }
    if (same && base && is_pinned(base + lo, hi - lo)) {
      CBFT_HIP(hipMemcpyAsync(din + lo, base + lo, hi - lo, hipMemcpyHostToDevice, cps));
      for (int k = 0; k < 5; k++) parts[k].bytes = 0;  // moved
    }
  }
  bool pageable_queued = false;  // copies still reading the caller's pageable memory
  if (!pack) {
    for (int k = 0; k < 5; k++)
      if (parts[k].bytes && !pinned[k]) {
        CBFT_HIP(hipMemcpyAsync(din + parts[k].off, parts[k].src, parts[k].bytes, hipMemcpyHostToDevice, cps));
        pageable_queued = true;
      }
  }
  if (phi) {
    CBFT_HIP(s.pack.reserve(in_bytes));
    for (int k = 0; k < 5; k++)
      if (parts[k].bytes && !pinned[k]) std::memcpy(s.pack.as<uint8_t>(parts[k].off), parts[k].src, parts[k].bytes);
    CBFT_HIP(hipMemcpyAsync(din + plo, s.pack.as<uint8_t>(plo), phi - plo, hipMemcpyHostToDevice, cps));
  }
  // pinned parts after the packed run (stream order: they win where the run spans them)
  for (int k = 0; k < 5; k++)
    if (parts[k].bytes && pinned[k])
      CBFT_HIP(hipMemcpyAsync(din + parts[k].off, parts[k].src, parts[k].bytes, hipMemcpyHostToDevice, cps));
  if (!one_stream) {
    CBFT_HIP(hipEventRecord(s.copied, cps));
    // the header's contract: pageable inputs may be reused as soon as the call returns, so a
    // batch whose pageable parts were not packed returns only after their copies completed (the
    // runtime may still be staging from the caller's memory)
    if (pageable_queued) CBFT_HIP(hipEventSynchronize(s.copied));
    CBFT_HIP(hipStreamWaitEvent(cs, s.copied, 0));
  }
  rc = launch_locked(c, table_id, kt ? nullptr : din + o_key, kt ? reinterpret_cast<const uint32_t*>(din + o_key) : nullptr,
                     din + o_sig, din + o_msg - mbase, fixed ? nullptr : reinterpret_cast<const uint64_t*>(din + o_off),
                     fixed ? nullptr : reinterpret_cast<const uint32_t*>(din + o_len), fixed_len, n,
                     s.verd.as<uint64_t>(), cs, uniform_blocks);
  if (rc) return rc;
  CBFT_HIP(hipMemcpyAsync(s.hverd.p, s.verd.p, nw * 8, hipMemcpyDeviceToHost, cs));
  CBFT_HIP(hipEventRecord(s.done, cs));
  s.ticket = t;
  s.pending = true;
  s.status = CBFT_OK;
  s.n = n;
  s.bitmap = bitmap;
  *ticket = t;
  return CBFT_OK;
}

static int wait_one(cbft_ctx* c, uint64_t ticket) {
  HostSlot& s = c->hslots[ticket % CBFT_HOST_SLOTS];
  std::lock_guard<std::mutex> g(s.m);
  if (s.ticket != ticket) return CBFT_OK;  // delivered when a later batch took the slot
  (void)hipSetDevice(c->device);
  return collect_locked(s);
}

// Multi-GPU context: static contiguous shards, boundaries on whole verdict words (64
// signatures) so each device writes whole bytes of the caller's bitmap; one async batch per
// device, all in flight together.
static int group_submit(cbft_ctx* c, uint32_t table_id, const uint8_t* pk, const uint32_t* key_idx, const uint8_t* sig,
                        const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len, bool fixed,
                        uint32_t fixed_len, size_t n, uint8_t* bitmap, uint64_t* ticket) {
  const size_t G = c->kids.size();
  const size_t per = (((n + G - 1) / G) + 63) / 64 * 64;
  std::vector<std::pair<size_t, uint64_t>> tk;
  int rc = CBFT_OK;
  for (size_t gi = 0; gi < G && rc == CBFT_OK; gi++) {
    const size_t lo = gi * per;
    if (lo >= n) break;
    const size_t m = std::min(n, lo + per) - lo;
    uint64_t kt = 0;
    rc = submit_host(c->kids[gi], table_id, pk ? pk + lo * 32 : nullptr, key_idx ? key_idx + lo : nullptr, sig + lo * 64,
                     fixed ? (msg_blob ? msg_blob + lo * (size_t)fixed_len : nullptr) : msg_blob,
                     fixed ? nullptr : msg_off + lo, fixed ? nullptr : msg_len + lo, fixed, fixed_len, m, bitmap + lo / 8,
                     &kt);
    if (rc == CBFT_OK) tk.emplace_back(gi, kt);
  }
  if (rc != CBFT_OK) {
    for (auto& p : tk) (void)wait_one(c->kids[p.first], p.second);
    return rc;
  }
  std::lock_guard<std::mutex> g(c->group_mu);
  const uint64_t t = ++c->next_ticket;
  c->group_tickets[t] = std::move(tk);
  *ticket = t;
  return CBFT_OK;
}

static int submit_any(cbft_ctx* c, uint32_t table_id, const uint8_t* pk, const uint32_t* key_idx, const uint8_t* sig,
                      const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len, bool fixed,
                      uint32_t fixed_len, size_t n, uint8_t* bitmap, uint64_t* ticket) {
  if (!c || !ticket || (n && (!sig || !bitmap || (!fixed && (!msg_off || !msg_len))))) return CBFT_EINVAL;
  *ticket = 0;
  if (n == 0) return CBFT_OK;
  if (!c->kids.empty())
    return group_submit(c, table_id, pk, key_idx, sig, msg_blob, msg_off, msg_len, fixed, fixed_len, n, bitmap, ticket);
  return submit_host(c, table_id, pk, key_idx, sig, msg_blob, msg_off, msg_len, fixed, fixed_len, n, bitmap, ticket);
}

int cbft_wait(cbft_ctx* c, uint64_t ticket) {
  if (!c) return CBFT_EINVAL;
  if (ticket == 0) return CBFT_OK;  // an empty batch
  if (c->kids.empty()) return wait_one(c, ticket);
  std::vector<std::pair<size_t, uint64_t>> tk;
  {
    std::lock_guard<std::mutex> g(c->group_mu);
    auto it = c->group_tickets.find(ticket);
    if (it == c->group_tickets.end()) return CBFT_OK;  // already waited
    tk = std::move(it->second);
    c->group_tickets.erase(it);
  }
  int rc = CBFT_OK;
  for (auto& p : tk) {
    const int r = wait_one(c->kids[p.first], p.second);
    if (r && !rc) rc = r;
  }
  return rc;
}

int cbft_ed25519_verify_batch_async(cbft_ctx* c, uint32_t table_id, const uint32_t* key_idx, const uint8_t* sig,
                                    const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len, size_t n,
                                    uint8_t* bitmap, uint64_t* ticket) {
  if (table_id == CBFT_NO_KEY_TABLE) return CBFT_EINVAL;
  return submit_any(c, table_id, nullptr, key_idx, sig, msg_blob, msg_off, msg_len, false, 0, n, bitmap, ticket);
}

int cbft_ed25519_verify_fixed_async(cbft_ctx* c, uint32_t table_id, const uint32_t* key_idx, const uint8_t* sig,
                                    const uint8_t* msg_blob, uint32_t msg_len, size_t n, uint8_t* bitmap,
                                    uint64_t* ticket) {
  if (table_id == CBFT_NO_KEY_TABLE) return CBFT_EINVAL;
  return submit_any(c, table_id, nullptr, key_idx, sig, msg_blob, nullptr, nullptr, true, msg_len, n, bitmap, ticket);
}

int cbft_ed25519_verify_batch(cbft_ctx* c, uint32_t table_id, const uint32_t* key_idx, const uint8_t* sig,
                              const uint8_t* msg_blob, const uint64_t* msg_off, const uint32_t* msg_len, size_t n,
                              uint8_t* bitmap) {
  uint64_t t = 0;
  int rc = cbft_ed25519_verify_batch_async(c, table_id, key_idx, sig, msg_blob, msg_off, msg_len, n, bitmap, &t);
  return rc ? rc : cbft_wait(c, t);
}

int cbft_ed25519_verify_batch_pk(cbft_ctx* c, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg_blob,
                                 const uint64_t* msg_off, const uint32_t* msg_len, size_t n, uint8_t* bitmap) {
  if (n && !pk) return CBFT_EINVAL;
  uint64_t t = 0;
  int rc = submit_any(c, CBFT_NO_KEY_TABLE, pk, nullptr, sig, msg_blob, msg_off, msg_len, false, 0, n, bitmap, &t);
  return rc ? rc : cbft_wait(c, t);
}

int cbft_ed25519_batch_layout(size_t n, uint32_t msg_len, size_t* off_key_idx, size_t* off_sig, size_t* off_msg,
                              size_t* total_bytes) {
  if (!off_key_idx || !off_sig || !off_msg || !total_bytes) return CBFT_EINVAL;
  BatchLayout l;
  batch_layout(n, true, true, l);
  *off_key_idx = l.key;
  *off_sig = l.sig;
  *off_msg = l.msg;
  *total_bytes = l.msg + (size_t)msg_len * n;
  return CBFT_OK;
}

int cbft_host_alloc(cbft_ctx* c, size_t bytes, void** out) {
  if (!c || !out || !bytes) return CBFT_EINVAL;
  *out = nullptr;
  CBFT_HIP(hipSetDevice(c->kids.empty() ? c->device : c->kids[0]->device));
  void* p = nullptr;
  CBFT_HIP(hipHostMalloc(&p, bytes, hipHostMallocPortable));  // DMA-able by every device
  {
    std::lock_guard<std::mutex> g(g_pin_mu);
    g_pinned[(uintptr_t)p] = bytes;
  }
  *out = p;
  return CBFT_OK;
}

int cbft_host_free(cbft_ctx* c, void* p) {
  if (!c || !p) return CBFT_EINVAL;
  {
    std::lock_guard<std::mutex> g(g_pin_mu);
    auto it = g_pinned.find((uintptr_t)p);
    if (it == g_pinned.end()) return CBFT_EINVAL;
    g_pinned.erase(it);
  }
  CBFT_HIP(hipHostFree(p));
  return CBFT_OK;
}

int cbft_ed25519_verify_batch_device(cbft_ctx* c, uint32_t table_id, const uint8_t* d_pk, const uint32_t* d_key_idx,
                                     const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_off,
                                     const uint32_t* d_len, size_t n, uint64_t* d_verdicts, void* stream) {
  if (!c || (n && (!d_sig || !d_off || !d_len || !d_verdicts))) return CBFT_EINVAL;
  if (table_id == CBFT_NO_KEY_TABLE && n && !d_pk) return CBFT_EINVAL;
  if (!c->kids.empty()) return CBFT_EINVAL;  // device pointers belong to one GPU: use its own context
  if (n == 0) return CBFT_OK;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  return launch_locked(c, table_id, d_pk, d_key_idx, d_sig, d_msg, d_off, d_len, 0, n, d_verdicts, s);
}

int cbft_ed25519_verify_fixed_device(cbft_ctx* c, uint32_t table_id, const uint8_t* d_pk, const uint32_t* d_key_idx,
                                     const uint8_t* d_sig, const uint8_t* d_msg, uint32_t msg_len, size_t n,
                                     uint64_t* d_verdicts, void* stream) {
  if (!c || (n && (!d_sig || !d_verdicts || (msg_len && !d_msg)))) return CBFT_EINVAL;
  if (table_id == CBFT_NO_KEY_TABLE && n && !d_pk) return CBFT_EINVAL;
  if (!c->kids.empty()) return CBFT_EINVAL;  // device pointers belong to one GPU: use its own context
  if (n == 0) return CBFT_OK;
  std::lock_guard<std::mutex> g(c->mu);
  CBFT_HIP(hipSetDevice(c->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  return launch_locked(c, table_id, d_pk, d_key_idx, d_sig, d_msg, nullptr, nullptr, msg_len, n, d_verdicts, s);
}

}  // extern "C"
