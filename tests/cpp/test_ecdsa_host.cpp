// Host-side test of concord::hip::HipECDSAVerifier (hip_crypto.hpp): keys from hex DER and from PEM,
// verify() and verifyBatch() against the host OpenSSL, wrong-length signatures, and a secp384r1 key
// on the host path.  `--no-gpu` runs the parts that need no GPU (parsing, the host path that other
// curves and secp256k1 calls below gpuMinBatch() take, the length rule); without it
// $CBFT_ECDSA_GPU_MIN is set to 1 so that every secp256k1 verification, lone ones included, runs on
// the GPU.
#include <openssl/bio.h>
#include <openssl/ec.h>
#include <openssl/ecdsa.h>
#include <openssl/evp.h>
#include <openssl/pem.h>
#include <openssl/x509.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "hip_crypto.hpp"

using namespace concord::hip;

static int g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      g_fail++;                                                   \
    }                                                             \
  } while (0)

struct Key {
  EVP_PKEY* pkey;
  std::string hex, pem;
};

static Key makeKey(const char* curve) {
  Key k;
  k.pkey = EVP_EC_gen(curve);
  if (!k.pkey) throw std::runtime_error("EVP_EC_gen");
  unsigned char* der = nullptr;
  const int n = i2d_PUBKEY(k.pkey, &der);
  if (n <= 0) throw std::runtime_error("i2d_PUBKEY");
  k.hex = toHex(der, (size_t)n);
  OPENSSL_free(der);
  BIO* bio = BIO_new(BIO_s_mem());
  PEM_write_bio_PUBKEY(bio, k.pkey);
  char* p = nullptr;
  const long pl = BIO_get_mem_data(bio, &p);
  k.pem.assign(p, (size_t)pl);
  BIO_free(bio);
  return k;
}

// r || s (each `half` bytes) over SHA-256, signed by the host OpenSSL
static std::string signP1363(EVP_PKEY* k, const std::string& msg, size_t half) {
  EVP_MD_CTX* md = EVP_MD_CTX_new();
  size_t dl = 0;
  if (EVP_DigestSignInit(md, nullptr, EVP_sha256(), nullptr, k) != 1 ||
      EVP_DigestSign(md, nullptr, &dl, (const unsigned char*)msg.data(), msg.size()) != 1)
    throw std::runtime_error("EVP_DigestSign");
  std::vector<unsigned char> der(dl);
  if (EVP_DigestSign(md, der.data(), &dl, (const unsigned char*)msg.data(), msg.size()) != 1)
    throw std::runtime_error("EVP_DigestSign");
  EVP_MD_CTX_free(md);
  const unsigned char* p = der.data();
  ECDSA_SIG* es = d2i_ECDSA_SIG(nullptr, &p, (long)dl);
  if (!es) throw std::runtime_error("d2i_ECDSA_SIG");
  std::string out(2 * half, '\0');
  BN_bn2binpad(ECDSA_SIG_get0_r(es), (unsigned char*)&out[0], (int)half);
  BN_bn2binpad(ECDSA_SIG_get0_s(es), (unsigned char*)&out[half], (int)half);
  ECDSA_SIG_free(es);
  return out;
}

// the host OpenSSL's verdict on r || s
static bool opensslVerify(EVP_PKEY* k, const std::string& msg, const std::string& sig) {
  const size_t half = sig.size() / 2;
  ECDSA_SIG* es = ECDSA_SIG_new();
  ECDSA_SIG_set0(es, BN_bin2bn((const unsigned char*)sig.data(), (int)half, nullptr),
                 BN_bin2bn((const unsigned char*)sig.data() + half, (int)half, nullptr));
  unsigned char* der = nullptr;
  const int dl = i2d_ECDSA_SIG(es, &der);
  ECDSA_SIG_free(es);
  bool ok = false;
  if (dl > 0) {
    EVP_MD_CTX* md = EVP_MD_CTX_new();
    ok = EVP_DigestVerifyInit(md, nullptr, EVP_sha256(), nullptr, k) == 1 &&
         EVP_DigestVerify(md, der, (size_t)dl, (const unsigned char*)msg.data(), msg.size()) == 1;
    EVP_MD_CTX_free(md);
  }
  OPENSSL_free(der);
  return ok;
}

template <class F>
static bool throwsInvalid(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  } catch (...) {
  }
  return false;
}

static void gpuFreeChecks(Key& k1, Key& k384) {
  HipECDSAVerifier a(k1.hex, KeyFormat::HexaDecimalStrippedFormat), b(k1.pem, KeyFormat::PemFormat);
  CHECK(a.gpuCapable() && b.gpuCapable());
  CHECK(a.signatureLength() == 64 && b.signatureLength() == 64);
  CHECK(a.engineKeyIndex() == b.engineKeyIndex());  // the same key registers once
  CHECK(a.getPubKey() == k1.hex && b.getPubKey() == k1.pem);
  // wrong-length signatures are false without a GPU call, never an exception
  const std::string good = signP1363(k1.pkey, "length rule", 32);
  CHECK(!a.verify("length rule", good.substr(0, 63)));
  CHECK(!a.verify("length rule", good + std::string(1, '\0')));
  CHECK(!a.verify("length rule", ""));
  if (HipECDSAVerifier::gpuMinBatch() > 1) {  // a lone secp256k1 verify() stays on the host
    CHECK(a.verify("length rule", good) && b.verify("length rule", good) && !a.verify("length rule!", good));
    std::string twisted = good;
    twisted[40] ^= 4;
    CHECK(!a.verify("length rule", twisted));
  }

  HipECDSAVerifier h(k384.hex, KeyFormat::HexaDecimalStrippedFormat), hp(k384.pem, KeyFormat::PemFormat);
  CHECK(!h.gpuCapable() && !hp.gpuCapable());
  CHECK(h.signatureLength() == 96);
  for (int i = 0; i < 8; i++) {
    const std::string msg = "secp384r1 on the host " + std::to_string(i);
    std::string sig = signP1363(k384.pkey, msg, 48);
    CHECK(h.verify(msg, sig) && hp.verify(msg, sig));
    CHECK(!h.verify(msg + "x", sig));
    sig[(size_t)(11 * i) % 96] ^= 0x20;
    CHECK(h.verify(msg, sig) == opensslVerify(k384.pkey, msg, sig));
    CHECK(!h.verify(msg, sig.substr(0, 64)));  // a secp256k1-sized signature under a secp384r1 key
  }
  std::vector<bool> out;
  const std::string m = "batch on the host", s = signP1363(k384.pkey, m, 48);
  std::vector<VerifyRequest> reqs{{&h, m.data(), m.size(), s.data(), s.size()},
                                  {&h, m.data(), m.size() - 1, s.data(), s.size()},
                                  {&a, m.data(), m.size(), s.data(), s.size()}};  // 96 bytes under a k1 key
  HipECDSAVerifier::verifyBatch(reqs, out);
  CHECK(out.size() == 3 && out[0] && !out[1] && !out[2]);

  CHECK(throwsInvalid([] { HipECDSAVerifier v("zz", KeyFormat::HexaDecimalStrippedFormat); }));
  CHECK(throwsInvalid([] { HipECDSAVerifier v("", KeyFormat::PemFormat); }));
  CHECK(throwsInvalid([&] { HipECDSAVerifier v(k1.hex.substr(0, k1.hex.size() - 2), KeyFormat::HexaDecimalStrippedFormat); }));
  EVP_PKEY* rsa = EVP_RSA_gen(2048);
  unsigned char* der = nullptr;
  const int n = i2d_PUBKEY(rsa, &der);
  const std::string rsa_hex = toHex(der, (size_t)n);
  OPENSSL_free(der);
  EVP_PKEY_free(rsa);
  CHECK(throwsInvalid([&] { HipECDSAVerifier v(rsa_hex, KeyFormat::HexaDecimalStrippedFormat); }));
}

static void gpuChecks(Key& k384) {
  std::vector<Key> keys;
  std::vector<std::unique_ptr<HipECDSAVerifier>> ver;
  for (int i = 0; i < 5; i++) {
    keys.push_back(makeKey("secp256k1"));
    ver.emplace_back(new HipECDSAVerifier(i & 1 ? keys[i].pem : keys[i].hex,
                                          i & 1 ? KeyFormat::PemFormat : KeyFormat::HexaDecimalStrippedFormat));
    CHECK(ver.back()->gpuCapable());
  }
  HipECDSAVerifier h(k384.hex, KeyFormat::HexaDecimalStrippedFormat);
  const size_t n = 200;
  std::vector<std::string> msgs(n), sigs(n);
  std::vector<const HipECDSAVerifier*> who(n);
  std::vector<bool> want(n);
  std::vector<VerifyRequest> reqs;
  for (size_t i = 0; i < n; i++) {
    msgs[i] = std::string(i % 150, (char)('a' + i % 26)) + std::to_string(i);
    if (i % 17 == 5) {  // a host-path item in the middle of the batch
      who[i] = &h;
      sigs[i] = signP1363(k384.pkey, msgs[i], 48);
      if (i % 2) sigs[i][7] ^= 1;
      want[i] = opensslVerify(k384.pkey, msgs[i], sigs[i]);
    } else {
      const size_t ki = i % keys.size();
      who[i] = ver[ki].get();
      sigs[i] = signP1363(keys[ki].pkey, msgs[i], 32);
      if (i % 7 == 3) sigs[i][(i * 5) % 64] ^= (char)(1 << (i % 8));
      if (i % 11 == 4) msgs[i] += "!";
      const size_t vk = i % 13 == 6 ? (ki + 1) % keys.size() : ki;  // verified under another key
      who[i] = ver[vk].get();
      want[i] = opensslVerify(keys[vk].pkey, msgs[i], sigs[i]);
    }
    reqs.push_back({who[i], msgs[i].data(), msgs[i].size(), sigs[i].data(), sigs[i].size()});
  }
  size_t accepted = 0;
  for (bool w : want) accepted += w;
  CHECK(accepted > n / 2 && accepted < n);
  std::vector<bool> out;
  HipECDSAVerifier::verifyBatch(reqs, out);
  CHECK(out.size() == n);
  for (size_t i = 0; i < n; i++) CHECK(out[i] == want[i]);
  concord::hip::verifyBatch(reqs, out);  // the mixed-batch dispatcher takes the same route
  for (size_t i = 0; i < n; i++) CHECK(out[i] == want[i]);
  for (size_t i = 0; i < 40; i++) CHECK(who[i]->verify(msgs[i], sigs[i]) == want[i]);
  // high-s twin: no low-s rule
  {
    const std::string m = "twin", s = signP1363(keys[0].pkey, m, 32);
    BIGNUM *order = BN_new(), *sv = BN_bin2bn((const unsigned char*)s.data() + 32, 32, nullptr);
    BN_hex2bn(&order, "FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141");
    BN_sub(sv, order, sv);
    std::string t = s;
    BN_bn2binpad(sv, (unsigned char*)&t[32], 32);
    BN_free(order);
    BN_free(sv);
    CHECK(ver[0]->verify(m, s) && ver[0]->verify(m, t) && opensslVerify(keys[0].pkey, m, t));
  }
  // a key registered after the table was built is picked up by the next batch
  Key late = makeKey("secp256k1");
  HipECDSAVerifier lv(late.hex, KeyFormat::HexaDecimalStrippedFormat);
  const std::string lm = "late key", ls = signP1363(late.pkey, lm, 32);
  CHECK(lv.verify(lm, ls) && !ver[0]->verify(lm, ls));
  EVP_PKEY_free(late.pkey);
  for (Key& k : keys) EVP_PKEY_free(k.pkey);
}

int main(int argc, char** argv) {
  const bool no_gpu = argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0;
  if (!no_gpu) setenv("CBFT_ECDSA_GPU_MIN", "1", 0);  // read once, at the first verify
  try {
    Key k1 = makeKey("secp256k1"), k384 = makeKey("secp384r1");
    gpuFreeChecks(k1, k384);
    if (!no_gpu) gpuChecks(k384);
    EVP_PKEY_free(k1.pkey);
    EVP_PKEY_free(k384.pkey);
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 2;
  }
  if (g_fail) {
    std::printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf(no_gpu ? "all GPU-free checks passed\n" : "all checks passed\n");
  return 0;
}
