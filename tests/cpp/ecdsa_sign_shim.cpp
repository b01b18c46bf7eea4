// Host build of the ECDSA secp256k1 signing lane code (concord-bft_amd/csrc/ecdsa_sign.h over
// ecdsa_verify.h's field, scalar, point and SHA-256 code), exposed to the Python tests through
// ctypes: the SAME source that runs on gfx950, checked on the CPU against tests/ecdsa_sign_ref.py
// and the golden vectors.  Test infrastructure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "ecdsa_sign.h"

namespace {
const uint32_t* comb_table() {
  static std::vector<uint32_t> tbl;
  if (tbl.empty()) {
    tbl.assign(ECDSAS_TABLE_WORDS, 0);
    for (int j = 0; j < ECDSAS_TABLE_LANES; j++) ecdsas_table_lane(tbl.data(), j);
  }
  return tbl.data();
}
void digest_words(uint32_t* h, const uint8_t* d32) {
  for (int i = 0; i < 8; i++)
    h[i] = ((uint32_t)d32[4 * i] << 24) | ((uint32_t)d32[4 * i + 1] << 16) | ((uint32_t)d32[4 * i + 2] << 8) | d32[4 * i + 3];
}
// 64 zero bytes and 0 under an unusable key, as the kernel does
int sign_words(uint8_t* out, const uint8_t* priv, const uint32_t* h) {
  uint32_t rec[ECDSAS_WORDS], sig[16];
  ecdsas_signer_lane(rec, priv, comb_table());
  if (!rec[ECDSAS_OK]) {
    std::memset(out, 0, 64);
    return 0;
  }
  ecdsas_sign_lane(sig, rec, h, comb_table());
  std::memcpy(out, sig, 64);
  return 1;
}
}  // namespace

extern "C" {

int ecdsa_sign_shim_table_words() { return ECDSAS_TABLE_WORDS; }
void ecdsa_sign_shim_table(uint32_t* out) { std::memcpy(out, comb_table(), ECDSAS_TABLE_WORDS * sizeof(uint32_t)); }

int ecdsa_sign_shim_sign(const uint8_t* priv, const uint8_t* msg, uint32_t len, uint8_t* out) {
  uint32_t h[8];
  ecdsa_sha256(h, msg, len);
  return sign_words(out, priv, h);
}
int ecdsa_sign_shim_sign_digest(const uint8_t* priv, const uint8_t* digest, uint8_t* out) {
  uint32_t h[8];
  digest_words(h, digest);
  return sign_words(out, priv, h);
}
// n fixed-length messages under keys priv[idx[i]] (idx null: key 0), over `threads` threads
void ecdsa_sign_shim_sign_many(const uint8_t* priv, const uint32_t* idx, const uint8_t* msg, uint32_t len, size_t n,
                               uint8_t* out, int threads) {
  (void)comb_table();
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++)
    th.emplace_back([=] {
      for (size_t i = t; i < n; i += threads)
        ecdsa_sign_shim_sign(priv + 32 * (size_t)(idx ? idx[i] : 0), msg + (size_t)len * i, len, out + 64 * i);
    });
  for (auto& x : th) x.join();
}
// the RFC 6979 nonce for the order q; returns the number of candidates refused
uint32_t ecdsa_sign_shim_nonce(const uint8_t* x, const uint8_t* digest, const uint8_t* q, uint8_t* out_k) {
  uint32_t xl[8], ql[8], h[8], k[8];
  k1_from_be(xl, x);
  k1_from_be(ql, q);
  digest_words(h, digest);
  const uint32_t refused = ecdsas_nonce(k, xl, h, ql);
  k1_to_be(out_k, k);
  return refused;
}
// the same after `skip` usable candidates were refused
uint32_t ecdsa_sign_shim_nonce_skip(const uint8_t* x, const uint8_t* digest, const uint8_t* q, uint32_t skip, uint8_t* out_k) {
  uint32_t xl[8], ql[8], h[8], k[8];
  k1_from_be(xl, x);
  k1_from_be(ql, q);
  digest_words(h, digest);
  const uint32_t refused = ecdsas_nonce_skip(k, xl, h, ql, skip);
  k1_to_be(out_k, k);
  return refused;
}
// 1 and r || s, or 0 ("next candidate": r = 0 or s = 0)
int ecdsa_sign_shim_sign_with_k(const uint8_t* x, const uint8_t* e, const uint8_t* k, uint8_t* out) {
  uint32_t xl[8], kl[8], sig[16];
  K1Sc el, r, s;
  k1_from_be(xl, x);
  k1_from_be(el.v, e);
  k1_from_be(kl, k);
  const uint32_t ok = ecdsas_sign_with_k(r, s, xl, el, kl, comb_table());
  ecdsas_put_sig(sig, r, s);
  std::memcpy(out, sig, 64);
  return ok ? 1 : 0;
}
// which: 0 = a^-1 mod p, 1 = a^-1 mod n (a below the modulus)
void ecdsa_sign_shim_inv(int which, const uint8_t* a, uint8_t* out) {
  if (which == 0) {
    K1Fe x, r;
    k1_from_be(x.v, a);
    fe_inv_ct(r, x);
    k1_to_be(out, r.v);
  } else {
    K1Sc x, r;
    k1_from_be(x.v, a);
    sc_inv_ct(r, x);
    k1_to_be(out, r.v);
  }
}
// k G for any 256-bit k as X || Y; returns 1 (and zeros) for infinity
int ecdsa_sign_shim_comb(const uint8_t* k, uint8_t* out) {
  uint32_t kl[8];
  k1_from_be(kl, k);
  K1Proj P;
  ecdsas_comb(P, kl, comb_table());
  K1Fe zi, x, y;
  fe_inv_ct(zi, P.z);
  fe_mul(x, P.x, zi);
  fe_mul(y, P.y, zi);
  k1_to_be(out, x.v);
  k1_to_be(out + 32, y.v);
  return fe_is_zero(P.z) ? 1 : 0;
}
void ecdsa_sign_shim_signer(const uint8_t* priv, uint32_t* rec) { ecdsas_signer_lane(rec, priv, comb_table()); }

}  // extern "C"

#ifdef ECDSA_SIGN_SHIM_MAIN
// The stand-alone form (ASan + UBSan): the x = 1 / "Satoshi Nakamoto" vector, an unusable key, the
// edge keys and nonces over every message length class.
int main() {
  static const uint8_t want[64] = {
      0x93, 0x4B, 0x1E, 0xA1, 0x0A, 0x4B, 0x3C, 0x17, 0x57, 0xE2, 0xB0, 0xC0, 0x17, 0xD0, 0xB6, 0x14,
      0x3C, 0xE3, 0xC9, 0xA7, 0xE6, 0xA4, 0xA4, 0x98, 0x60, 0xD7, 0xA6, 0xAB, 0x21, 0x0E, 0xE3, 0xD8,
      0xDB, 0xBD, 0x31, 0x62, 0xD4, 0x6E, 0x9F, 0x9B, 0xEF, 0x7F, 0xEB, 0x87, 0xC1, 0x6D, 0xC1, 0x3B,
      0x4F, 0x65, 0x68, 0xA8, 0x7F, 0x4E, 0x83, 0xF7, 0x28, 0xE2, 0x44, 0x3B, 0xA5, 0x86, 0x67, 0x5C};
  uint8_t priv[32] = {0}, out[64];
  priv[31] = 1;
  const char* m = "Satoshi Nakamoto";
  int bad = 0;
  if (ecdsa_sign_shim_sign(priv, reinterpret_cast<const uint8_t*>(m), 16, out) != 1 || std::memcmp(out, want, 64)) bad++;
  std::memset(priv, 0xFF, 32);  // x >= n
  if (ecdsa_sign_shim_sign(priv, reinterpret_cast<const uint8_t*>(m), 16, out) != 0) bad++;
  for (int i = 0; i < 64; i++) bad += out[i] != 0;
  std::vector<uint8_t> msg(4096);
  for (size_t i = 0; i < msg.size(); i++) msg[i] = (uint8_t)(i * 131 + 7);
  const uint32_t lens[] = {0, 1, 31, 32, 55, 56, 63, 64, 65, 119, 120, 256, 4096};
  for (uint32_t len : lens) {
    std::memset(priv, 0x88, 32);
    priv[0] = (uint8_t)len;
    if (ecdsa_sign_shim_sign(priv, msg.data(), len, out) != 1) bad++;
    uint8_t pt[64];
    bad += ecdsa_sign_shim_comb(priv, pt);
  }
  uint8_t zero[32] = {0}, pt[64];
  if (ecdsa_sign_shim_comb(zero, pt) != 1) bad++;
  std::printf(bad ? "FAILED: %d\n" : "signatures and rejections as expected (%d)\n", bad);
  return bad ? 1 : 0;
}
#endif
