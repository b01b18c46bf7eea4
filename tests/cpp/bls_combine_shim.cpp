// Host build of the batched BLS combination lane code (concord-bft_amd/csrc/bls_combine_batch.h): the
// SAME source that runs one share per lane on gfx950, exposed to tests/test_bls_combine_batch_cpu.py
// through ctypes, and (-DBLS_COMBINE_SHIM_MAIN) a stand-alone self-check for a sanitizer build.  The
// kernels' glue (decoding, the wave's segmented butterfly) is restated here on plain arrays.  Test
// infrastructure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bls_combine_batch.h"

static const uint32_t* inv_table() {
  static std::vector<uint32_t> t;
  if (t.empty()) {
    t.resize((size_t)BLS_COMBINE_INV * BN_LIMBS);
    for (uint32_t d = 1; d <= BLS_COMBINE_INV; d++) {
      const uint32_t w[8] = {d, 0, 0, 0, 0, 0, 0, 0};
      fr x;
      f_from_words(x, w);
      fr_inv(x, x);
      for (int q = 0; q < BN_LIMBS; q++) t[BN_LIMBS * (size_t)(d - 1) + q] = x.v[q];
    }
  }
  return t.data();
}

static void id_mont(uint32_t* out9, uint32_t id) {
  const uint32_t w[8] = {id, 0, 0, 0, 0, 0, 0, 0};
  fr t;
  f_from_words(t, w);
  for (int q = 0; q < BN_LIMBS; q++) out9[q] = t.v[q];
}

extern "C" {

// Stage 2 over one certificate of k ids: lam (k x 32 bytes big-endian, written for the good shares whose
// id nobody repeats), state (k: BLSC_*) and dup (k: the walk met the id again).  use nullable.
void blsc_shim_lagrange(const uint32_t* ids, const uint8_t* use, uint32_t k, uint8_t* lam, uint8_t* state,
                        uint8_t* dup) {
  std::vector<uint32_t> idm((size_t)k * BN_LIMBS);
  for (uint32_t j = 0; j < k; j++) {
    const bool used = use ? use[j] != 0 : true;
    state[j] = !used ? BLSC_UNUSED : (ids[j] >= 1 && ids[j] <= BLS_COMBINE_MAX_K ? BLSC_GOOD : BLSC_BAD);
    if (state[j] == BLSC_GOOD) id_mont(&idm[BN_LIMBS * (size_t)j], ids[j]);
  }
  for (uint32_t i = 0; i < k; i++) {
    dup[i] = 0;
    if (state[i] != BLSC_GOOD) continue;
    uint32_t l8[8];
    if (blsc_lagrange_lane(l8, ids, idm.data(), state, 0, k, i, inv_table(), false))
      dup[i] = 1;
    else
      words_to_be32(lam + 32 * (size_t)i, l8);
  }
}

// Stage 3 on one point: out33 = compress(k * P); -1 when p33 does not decode
int blsc_shim_mul(const uint8_t* p33, const uint8_t* kbe, uint8_t* out33) {
  g1a P, a;
  if (!g1_decompress(P, p33)) return -1;
  uint32_t k[8];
  be32_to_words(k, kbe);
  BlsTblLocal tbl;
  g1j R;
  blsc_mul_lane(R, P, k, tbl);
  g1_to_affine<true>(a, R);
  g1_compress(out33, a);
  return 0;
}

// The whole launch sequence on the host: n shares, m certificates at off[0 .. m] (off[0] = 0, off[m] = n)
void blsc_shim_batch(const uint8_t* shares37, uint32_t n, const uint32_t* off, uint32_t m, const uint8_t* use,
                     int multisig, uint8_t* out33, uint8_t* status) {
  std::vector<uint8_t> state(n);
  std::vector<uint32_t> ids(n), idm((size_t)n * BN_LIMBS), flag(n), cert(n);
  std::vector<g1a> sig(n);
  std::vector<g1j> prod(n);
  for (uint32_t c = 0; c < m; c++)
    for (uint32_t j = off[c]; j < off[c + 1]; j++) cert[j] = c;
  for (uint32_t j = 0; j < n; j++) {  // stage 1
    const bool used = use ? use[j] != 0 : true;
    uint32_t id = 0;
    const bool ok = used && bls_parse_share(id, sig[j], shares37 + 37 * (size_t)j);
    state[j] = !used ? BLSC_UNUSED : (ok && id >= 1 && id <= BLS_COMBINE_MAX_K ? BLSC_GOOD : BLSC_BAD);
    if (state[j] == BLSC_GOOD) {
      ids[j] = id;
      id_mont(&idm[BN_LIMBS * (size_t)j], id);
    }
  }
  for (uint32_t i = 0; i < n; i++) {  // stages 2 and 3
    flag[i] = state[i] == BLSC_UNUSED ? 0u : BLSC_F_USED;
    if (state[i] == BLSC_BAD) flag[i] |= BLSC_F_BAD;
    g1_set_inf(prod[i]);
    if (state[i] != BLSC_GOOD) continue;
    uint32_t l8[8];
    if (blsc_lagrange_lane(l8, ids.data(), idm.data(), state.data(), off[cert[i]], off[cert[i] + 1], i, inv_table(),
                           multisig != 0)) {
      flag[i] |= BLSC_F_BAD;
    } else if (multisig) {
      g1_from_affine(prod[i], sig[i]);
    } else {
      BlsTblLocal tbl;
      blsc_mul_lane(prod[i], sig[i], l8, tbl);
    }
  }
  for (uint32_t base = 0; base < n; base += 64) {  // stage 4, the wave: every lane reads, then every lane adds
    const uint32_t cnt = n - base < 64 ? n - base : 64;
    for (uint32_t d = 1; d < 64; d <<= 1) {
      std::vector<g1j> old(prod.begin() + base, prod.begin() + base + cnt);
      std::vector<uint32_t> oldf(flag.begin() + base, flag.begin() + base + cnt);
      for (uint32_t l = 0; l + d < cnt; l++)
        if (cert[base + l + d] == cert[base + l]) {
          blsc_add(prod[base + l], old[l], old[l + d]);
          flag[base + l] = oldf[l] | oldf[l + d];
        }
    }
  }
  for (uint32_t c = 0; c < m; c++) {  // stage 4, the certificate
    const uint32_t lo = off[c], hi = off[c + 1];
    const uint32_t np = lo == hi ? 0u : 1u + ((hi - 1) / 64u - lo / 64u);
    auto at = [lo](uint32_t q) { return q ? (lo / 64u + q) * 64u : lo; };
    uint32_t f = 0;
    for (uint32_t q = 0; q < np; q++) f |= flag[at(q)];
    blsc_finish(out33 + 33 * (size_t)c, status + c, f, np, [&](g1j& p, uint32_t q) { p = prod[at(q)]; });
  }
}

}  // extern "C"

#ifdef BLS_COMBINE_SHIM_MAIN
static uint64_t sm64(uint64_t& x) {
  uint64_t z = (x += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// k * P by plain double-and-add (g1_mul), compressed
static void plain_mul(uint8_t* out33, const g1a& P, const uint32_t* k) {
  g1j J, R;
  g1_from_affine(J, P);
  g1_mul(R, J, k);
  g1a a;
  g1_to_affine<true>(a, R);
  g1_compress(out33, a);
}

int main() {
  int bad = 0;
  uint64_t st = 7;
  g1a H;
  g1_map(H, reinterpret_cast<const uint8_t*>("combine"), 7);
  uint8_t h33[33];
  g1_compress(h33, H);
  // stage 3 against double-and-add: small, top-bit and random scalars
  for (int t = 0; t < 24; t++) {
    uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (t < 4)
      k[0] = (uint32_t)t;
    else if (t == 4)
      k[3] = 0x80000000u;
    else
      for (int q = 0; q < 8; q++) k[q] = (uint32_t)sm64(st) >> (q == 7 ? 4 : 0);
    uint8_t kbe[32], a[33], b[33];
    words_to_be32(kbe, k);
    if (blsc_shim_mul(h33, kbe, a)) bad++;
    plain_mul(b, H, k);
    if (std::memcmp(a, b, 33)) bad++;
  }
  // one batch: shares s_j = j * H under ids 1 .. k stand for a sharing of the constant polynomial... any
  // points do: the combination must equal sum lambda_j s_j formed with g1_mul and blsc_shim_lagrange
  const uint32_t ks[4] = {1, 5, 0, 70};
  std::vector<uint8_t> sh;
  std::vector<uint32_t> off{0};
  for (uint32_t k : ks) {
    for (uint32_t j = 1; j <= k; j++) {
      uint32_t w[8] = {(uint32_t)sm64(st) | 1u, 0, 0, 0, 0, 0, 0, 0};
      uint8_t s[37] = {0, 0, (uint8_t)(j >> 8), (uint8_t)j};
      plain_mul(s + 4, H, w);
      sh.insert(sh.end(), s, s + 37);
    }
    off.push_back((uint32_t)(sh.size() / 37));
  }
  for (int multisig = 0; multisig < 2; multisig++) {
    uint8_t out[4 * 33], status[4];
    blsc_shim_batch(sh.data(), off[4], off.data(), 4, nullptr, multisig, out, status);
    for (int c = 0; c < 4; c++) {
      const uint32_t k = ks[c];
      if (status[c] != (k ? 1 : 0)) bad++;
      if (!k) continue;
      std::vector<uint32_t> ids(k);
      std::vector<uint8_t> lam(32 * k), state(k), dup(k);
      for (uint32_t j = 0; j < k; j++) ids[j] = j + 1;
      blsc_shim_lagrange(ids.data(), nullptr, k, lam.data(), state.data(), dup.data());
      g1j acc;
      g1_set_inf(acc);
      for (uint32_t j = 0; j < k; j++) {
        g1a s;
        if (!g1_decompress(s, &sh[37 * (size_t)(off[c] + j) + 4])) bad++;
        g1j J, T;
        g1_from_affine(J, s);
        if (!multisig) {
          uint32_t l8[8];
          be32_to_words(l8, &lam[32 * j]);
          g1_mul(T, J, l8);
          J = T;
        }
        g1_add(T, acc, J);
        acc = T;
      }
      g1a a;
      g1_to_affine<true>(a, acc);
      uint8_t want[33];
      g1_compress(want, a);
      if (std::memcmp(want, out + 33 * c, 33)) bad++;
    }
  }
  std::printf(bad ? "%d mismatches\n" : "all %d checks as expected\n", bad ? bad : 24 + 8);
  return bad ? 1 : 0;
}
#endif
