// Host build of the ECDSA P-256 signing lane code (concord-bft_amd/csrc/ecdsa_p256_sign.h over
// ecdsa_p256_verify.h's field, scalar and point code and ecdsa_sign.h's DRBG) and of the DER writer
// (ecdsa_der.h), exposed to the Python tests through ctypes: the SAME source that runs on gfx950,
// checked on the CPU against tests/p256_sign_ref.py and the golden vectors.  Test infrastructure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "ecdsa_der.h"
#include "ecdsa_p256_sign.h"

namespace {
const uint32_t* comb_table() {
  static std::vector<uint32_t> tbl;
  if (tbl.empty()) {
    std::vector<uint32_t> t(ECDSAS_TABLE_WORDS, 0);
    for (int j = 0; j < ECDSAS_TABLE_LANES; j++) p2s_table_lane(t.data(), j);
    tbl.swap(t);
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
  p2s_signer_lane(rec, priv, comb_table());
  if (!rec[ECDSAS_OK]) {
    std::memset(out, 0, 64);
    return 0;
  }
  p2s_sign_lane(sig, rec, h, comb_table());
  std::memcpy(out, sig, 64);
  return 1;
}
void fe_in(P2Fe& r, const uint8_t* b) { k1_from_be(r.v, b); }
}  // namespace

extern "C" {

int ecdsa_p256_sign_shim_table_words() { return ECDSAS_TABLE_WORDS; }
void ecdsa_p256_sign_shim_table(uint32_t* out) { std::memcpy(out, comb_table(), ECDSAS_TABLE_WORDS * sizeof(uint32_t)); }

int ecdsa_p256_sign_shim_sign(const uint8_t* priv, const uint8_t* msg, uint32_t len, uint8_t* out) {
  uint32_t h[8];
  ecdsa_sha256(h, msg, len);
  return sign_words(out, priv, h);
}
int ecdsa_p256_sign_shim_sign_digest(const uint8_t* priv, const uint8_t* digest, uint8_t* out) {
  uint32_t h[8];
  digest_words(h, digest);
  return sign_words(out, priv, h);
}
// the lane routine with the digest that seeds the generator and the reduced digest e that enters s given apart
// (x usable): what reaches the s = 0 retry
void ecdsa_p256_sign_shim_sign_digest_e(const uint8_t* priv, const uint8_t* digest, const uint8_t* e, uint8_t* out) {
  uint32_t xl[8], h[8], sig[16];
  P2Sc el;
  k1_from_be(xl, priv);
  k1_from_be(el.v, e);
  digest_words(h, digest);
  p2s_sign_lane_e(sig, xl, h, el, comb_table());
  std::memcpy(out, sig, 64);
}
// n fixed-length messages under keys priv[idx[i]] (idx null: key 0), over `threads` threads
void ecdsa_p256_sign_shim_sign_many(const uint8_t* priv, const uint32_t* idx, const uint8_t* msg, uint32_t len, size_t n,
                                    uint8_t* out, int threads) {
  (void)comb_table();
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++)
    th.emplace_back([=] {
      for (size_t i = t; i < n; i += threads)
        ecdsa_p256_sign_shim_sign(priv + 32 * (size_t)(idx ? idx[i] : 0), msg + (size_t)len * i, len, out + 64 * i);
    });
  for (auto& x : th) x.join();
}
// the RFC 6979 nonce for P-256's order after `skip` usable candidates were refused; returns the number refused
uint32_t ecdsa_p256_sign_shim_nonce_skip(const uint8_t* x, const uint8_t* digest, uint32_t skip, uint8_t* out_k) {
  const uint32_t N[8] = P2_N_LIMBS;
  uint32_t xl[8], h[8], k[8];
  k1_from_be(xl, x);
  digest_words(h, digest);
  const uint32_t refused = ecdsas_nonce_skip(k, xl, h, N, skip);
  k1_to_be(out_k, k);
  return refused;
}
// 1 and r || s, or 0 ("next candidate": r = 0 or s = 0) and r || s as computed
int ecdsa_p256_sign_shim_sign_with_k(const uint8_t* x, const uint8_t* e, const uint8_t* k, uint8_t* out) {
  uint32_t xl[8], kl[8], sig[16];
  P2Sc el, r, s;
  k1_from_be(xl, x);
  k1_from_be(el.v, e);
  k1_from_be(kl, k);
  const uint32_t ok = p2s_sign_with_k(r, s, xl, el, kl, comb_table());
  p2s_put_sig(sig, r, s);
  std::memcpy(out, sig, 64);
  return ok ? 1 : 0;
}
// which: 0 = a^-1 mod p, 1 = a^-1 mod n (a below the modulus)
void ecdsa_p256_sign_shim_inv(int which, const uint8_t* a, uint8_t* out) {
  if (which == 0) {
    P2Fe x, r;
    fe_in(x, a);
    p2s_fe_inv_ct(r, x);
    k1_to_be(out, r.v);
  } else {
    P2Sc x, r;
    k1_from_be(x.v, a);
    p2s_sc_inv_ct(r, x);
    k1_to_be(out, r.v);
  }
}
// b a mod p
void ecdsa_p256_sign_shim_mulb(const uint8_t* a, uint8_t* out) {
  P2Fe x, r;
  fe_in(x, a);
  p2s_fe_mulb(r, x);
  k1_to_be(out, r.v);
}
// x mod n for a field element x
void ecdsa_p256_sign_shim_x_mod_n(const uint8_t* x, uint8_t* out) {
  P2Fe a;
  P2Sc r;
  fe_in(a, x);
  p2s_x_mod_n(r, a);
  k1_to_be(out, r.v);
}
// the complete addition as it stands: p = X || Y || Z (any projective triple), q = x || y -> X3 || Y3 || Z3
void ecdsa_p256_sign_shim_madd(const uint8_t* p, const uint8_t* q, uint8_t* out) {
  P2Proj a, r;
  P2Fe qx, qy;
  fe_in(a.x, p);
  fe_in(a.y, p + 32);
  fe_in(a.z, p + 64);
  fe_in(qx, q);
  fe_in(qy, q + 32);
  p2s_madd(r, a, qx, qy);
  k1_to_be(out, r.x.v);
  k1_to_be(out + 32, r.y.v);
  k1_to_be(out + 64, r.z.v);
}
// k G for any 256-bit k as X || Y; returns 1 (and zeros) for infinity
int ecdsa_p256_sign_shim_comb(const uint8_t* k, uint8_t* out) {
  uint32_t kl[8];
  k1_from_be(kl, k);
  P2Proj P;
  p2s_comb(P, kl, comb_table());
  P2Fe zi, x, y;
  p2s_fe_inv_ct(zi, P.z);
  p2_fe_mul(x, P.x, zi);
  p2_fe_mul(y, P.y, zi);
  k1_to_be(out, x.v);
  k1_to_be(out + 32, y.v);
  return p2_fe_is_zero(P.z) ? 1 : 0;
}
void ecdsa_p256_sign_shim_signer(const uint8_t* priv, uint32_t* rec) { p2s_signer_lane(rec, priv, comb_table()); }

// r || s (2 x 32 bytes) -> DER; returns the length (0 on refusal)
int ecdsa_p256_sign_shim_rs_to_der(const uint8_t* rs, uint8_t* out) {
  size_t len = 0;
  uint8_t buf[ECDSA_DER_MAX_BYTES(32)];
  if (!ecdsa_rs_to_der(rs, 32, buf, &len)) return 0;
  std::memcpy(out, buf, len);
  return (int)len;
}
int ecdsa_p256_sign_shim_der_to_rs(const uint8_t* der, uint32_t len, uint8_t* out_rs) {
  return ecdsa_der_to_rs(der, len, 32, out_rs) ? 1 : 0;
}

}  // extern "C"

#ifdef ECDSA_P256_SIGN_SHIM_MAIN
// The stand-alone form (ASan + UBSan): RFC 6979 A.2.5 "sample" and "test", an unusable key, keys and
// nonces over every message length class, the comb's corners and the DER writer's widths.
static void unhex(uint8_t* out, const char* s, size_t n) {
  for (size_t i = 0; i < n; i++) {
    unsigned v;
    std::sscanf(s + 2 * i, "%2x", &v);
    out[i] = (uint8_t)v;
  }
}
int main() {
  uint8_t priv[32], want[64], out[64];
  unhex(priv, "C9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721", 32);
  int bad = 0;
  unhex(want,
        "EFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716"
        "F7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8",
        64);
  if (ecdsa_p256_sign_shim_sign(priv, reinterpret_cast<const uint8_t*>("sample"), 6, out) != 1 || std::memcmp(out, want, 64)) bad++;
  unhex(want,
        "F1ABB023518351CD71D881567B1EA663ED3EFCF6C5132B354F28D3B0B7D38367"
        "019F4113742A2B14BD25926B49C649155F267E60D3814B4C0CC84250E46F0083",
        64);
  if (ecdsa_p256_sign_shim_sign(priv, reinterpret_cast<const uint8_t*>("test"), 4, out) != 1 || std::memcmp(out, want, 64)) bad++;
  uint8_t der[ECDSA_DER_MAX_BYTES(32)], back[64];
  const int dl = ecdsa_p256_sign_shim_rs_to_der(out, der);
  if (dl <= 0 || !ecdsa_p256_sign_shim_der_to_rs(der, (uint32_t)dl, back) || std::memcmp(back, out, 64)) bad++;
  std::memset(priv, 0xFF, 32);  // x >= n
  if (ecdsa_p256_sign_shim_sign(priv, reinterpret_cast<const uint8_t*>("test"), 4, out) != 0) bad++;
  for (int i = 0; i < 64; i++) bad += out[i] != 0;
  std::vector<uint8_t> msg(4096);
  for (size_t i = 0; i < msg.size(); i++) msg[i] = (uint8_t)(i * 131 + 7);
  const uint32_t lens[] = {0, 1, 31, 32, 55, 56, 63, 64, 65, 119, 120, 256, 4096};
  for (uint32_t len : lens) {
    std::memset(priv, 0x88, 32);
    priv[0] = (uint8_t)len;
    if (ecdsa_p256_sign_shim_sign(priv, msg.data(), len, out) != 1) bad++;
    uint8_t pt[64];
    bad += ecdsa_p256_sign_shim_comb(priv, pt);
  }
  uint8_t zero[32] = {0}, pt[64];
  if (ecdsa_p256_sign_shim_comb(zero, pt) != 1) bad++;
  for (int width = 0; width <= 32; width++) {  // r, s with `width` leading zero bytes, top bit set and clear
    uint8_t rs[64];
    std::memset(rs, 0, 64);
    for (int i = width; i < 32; i++) rs[i] = rs[32 + i] = (uint8_t)(0x80 + i);
    if (width < 32) rs[32 + width] = 0x7F;
    const int n = ecdsa_p256_sign_shim_rs_to_der(rs, der);
    if (n <= 0 || !ecdsa_p256_sign_shim_der_to_rs(der, (uint32_t)n, back) || std::memcmp(back, rs, 64)) bad++;
  }
  std::printf(bad ? "FAILED: %d\n" : "signatures and rejections as expected (%d)\n", bad);
  return bad ? 1 : 0;
}
#endif
