// Host build of the batched BLS signing lane routine (concord-bft_amd/csrc/bls_sign_batch.h): the
// SAME source that runs one message per lane on gfx950, exposed to tests/test_bls_sign_cpu.py
// through ctypes.  Test infrastructure.
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "bls_sign_batch.h"

static uint64_t sm64(uint64_t& x) {
  uint64_t z = (x += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// a reduced element (normalised limbs, value < 2q) with the given top limb
static void fp_with_top(fp& r, uint32_t top, uint64_t& st) {
  for (int i = 0; i < BN_LIMBS - 1; i++) r.v[i] = (uint32_t)sm64(st) & BN_MASK;
  r.v[BN_LIMBS - 1] = top;
}
static bool limbs_eq(const fp& a, const fp& b) { return std::memcmp(a.v, b.v, sizeof(a.v)) == 0; }

// f_add_ct / f_sub_ct against f_add / f_sub, limb for limb, on one operand pair; *fixed counts the
// pairs whose result differs from the uncorrected pass (the correction pass ran)
static int addsub_pair(const fp& a, const fp& b, long* fixed) {
  fp s0, s1, d0, d1;
  f_add(s0, a, b);
  f_add_ct(s1, a, b);
  f_sub(d0, a, b);
  f_sub_ct(d1, a, b);
  uint32_t q2[BN_LIMBS];
  f_2q<FpParams>(q2);
  // did the signed pass of the addition / subtraction end negative?
  const uint32_t T = q2[BN_LIMBS - 1], t = a.v[BN_LIMBS - 1] + b.v[BN_LIMBS - 1];
  int64_t c = 0;
  for (int i = 0; i < BN_LIMBS; i++) c = ((int64_t)a.v[i] + b.v[i] - (t + 2 > T ? q2[i] : 0) + c) >> 29;
  if (c < 0) ++*fixed;
  c = 0;
  const bool add2q = a.v[BN_LIMBS - 1] < b.v[BN_LIMBS - 1];
  for (int i = 0; i < BN_LIMBS; i++) c = ((int64_t)a.v[i] - b.v[i] + (add2q ? q2[i] : 0) + c) >> 29;
  if (c < 0) ++*fixed;
  return (limbs_eq(s0, s1) ? 0 : 1) + (limbs_eq(d0, d1) ? 0 : 1);
}

extern "C" {

// `pairs` random reduced operand pairs: returns the mismatches
long bls_sign_shim_addsub_random(uint64_t seed, long pairs, long* fixed) {
  uint32_t q2[BN_LIMBS];
  f_2q<FpParams>(q2);
  const uint32_t T = q2[BN_LIMBS - 1];
  long bad = 0;
  *fixed = 0;
  for (long i = 0; i < pairs; i++) {
    fp a, b;
    fp_with_top(a, (uint32_t)(sm64(seed) % T), seed);
    fp_with_top(b, (uint32_t)(sm64(seed) % T), seed);
    bad += addsub_pair(a, b, fixed);
  }
  return bad;
}

// the top-limb ties: a8 + b8 in {T - 1, T} (the addition's 2q comes off before a + b is known to reach
// it) and a8 == b8 (the subtraction adds nothing before a < b is known); low limbs random, and set
// to 0 / all ones on one side to force both outcomes.  Returns the mismatches; *fixed = passes that
// ended negative and were corrected.
long bls_sign_shim_addsub_ties(uint64_t seed, long pairs, long* fixed) {
  uint32_t q2[BN_LIMBS];
  f_2q<FpParams>(q2);
  const uint32_t T = q2[BN_LIMBS - 1];
  long bad = 0;
  *fixed = 0;
  for (long i = 0; i < pairs; i++) {
    const uint32_t t = T - (uint32_t)(i & 1);
    const uint32_t a8 = 1 + (uint32_t)(sm64(seed) % (t - 1));
    fp a, b;
    fp_with_top(a, a8, seed);
    fp_with_top(b, t - a8, seed);
    if ((i & 6) == 2)
      for (int k = 0; k < BN_LIMBS - 1; k++) a.v[k] = b.v[k] = 0;
    if ((i & 6) == 4)
      for (int k = 0; k < BN_LIMBS - 1; k++) a.v[k] = b.v[k] = BN_MASK;
    bad += addsub_pair(a, b, fixed);
    fp_with_top(b, a8, seed);  // equal top limbs
    bad += addsub_pair(a, b, fixed);
    bad += addsub_pair(b, a, fixed);
  }
  return bad;
}

// one share through bls_signer_record + bls_sign_lane<w> (w = 3 | 4; 0 = the window the product runs);
// sk 32 bytes big-endian in [1, r).  Returns the increments the hash needed.
int bls_sign_shim_share(int w, const uint8_t* skbe, uint32_t id, const uint8_t* msg, uint32_t len, uint8_t* out37) {
  uint32_t k[8], rec[BLS_SIGNER_WORDS];
  be32_to_words(k, skbe);
  bls_signer_record(rec, k, id);
  g1a H;
  int inc = 0;
  bls_map_x0(H.x, msg, len);
  while (!bls_map_try(H.y, H.x)) inc++;
  H.inf = false;
  BlsTblLocal tbl;
  if ((w ? w : BLS_SIGN_W) == 3)
    bls_sign_lane<3>(out37, H, rec, tbl);
  else
    bls_sign_lane<4>(out37, H, rec, tbl);
  return inc;
}

// n shares (message i = blob[off[i] .. + len[i]) under key sidx[i]) on host threads
void bls_sign_shim_shares_mt(int w, const uint8_t* sks, const uint32_t* ids, const uint32_t* sidx, const uint8_t* blob,
                             const uint64_t* off, const uint32_t* len, uint32_t n, uint8_t* out, int* incs,
                             int threads) {
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++)
    th.emplace_back([=] {
      for (uint32_t j = t; j < n; j += threads) {
        const uint32_t s = sidx ? sidx[j] : 0;
        const int inc = bls_sign_shim_share(w, sks + 32 * s, ids[s], blob + off[j], len[j], out + 37 * j);
        if (incs) incs[j] = inc;
      }
    });
  for (auto& x : th) x.join();
}

// the record of sk (BLS_SIGNER_WORDS words)
void bls_sign_shim_record(const uint8_t* skbe, uint32_t id, uint32_t* rec) {
  uint32_t k[8];
  be32_to_words(k, skbe);
  bls_signer_record(rec, k, id);
}

}  // extern "C"
