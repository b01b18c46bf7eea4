// Host-side test of concord::hip::HipECDSASigner (hip_crypto.hpp): keys from hex DER and from PEM,
// sign() against signBatch() on the GPU and on the host path, every signature accepted by
// HipECDSAVerifier and by the host OpenSSL, a secp384r1 key on the host path, the ecdsaSignStats()
// counters.  `--no-gpu` runs the parts that need no GPU (signBatch below gpuMinBatch() and on another
// curve is the host loop); without it $CBFT_ECDSA_SIGN_GPU_MIN is left at its default, so the batch
// of 40 runs on the GPU and the batch of 5 on the host.
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
  std::string hex, pem;  // the private key as PKCS#8: hex DER and PEM
};

static Key makeKey(const char* curve) {
  Key k;
  k.pkey = EVP_EC_gen(curve);
  if (!k.pkey) throw std::runtime_error("EVP_EC_gen");
  BIO* bio = BIO_new(BIO_s_mem());
  if (i2d_PKCS8PrivateKey_bio(bio, k.pkey, nullptr, nullptr, 0, nullptr, nullptr) != 1) throw std::runtime_error("i2d_PKCS8");
  char* p = nullptr;
  long pl = BIO_get_mem_data(bio, &p);
  k.hex = toHex(reinterpret_cast<const uint8_t*>(p), (size_t)pl);
  BIO_free(bio);
  bio = BIO_new(BIO_s_mem());
  if (PEM_write_bio_PrivateKey(bio, k.pkey, nullptr, nullptr, 0, nullptr, nullptr) != 1) throw std::runtime_error("PEM_write");
  pl = BIO_get_mem_data(bio, &p);
  k.pem.assign(p, (size_t)pl);
  BIO_free(bio);
  return k;
}

// the host OpenSSL's verdict on r || s over SHA-256
static bool opensslVerify(EVP_PKEY* k, const std::string& msg, const std::string& sig) {
  const size_t half = sig.size() / 2;
  ECDSA_SIG* es = ECDSA_SIG_new();
  BIGNUM* r = BN_bin2bn((const unsigned char*)sig.data(), (int)half, nullptr);
  BIGNUM* s = BN_bin2bn((const unsigned char*)sig.data() + half, (int)half, nullptr);
  ECDSA_SIG_set0(es, r, s);
  unsigned char* der = nullptr;
  const int dl = i2d_ECDSA_SIG(es, &der);
  EVP_MD_CTX* md = EVP_MD_CTX_new();
  const bool ok = dl > 0 && EVP_DigestVerifyInit(md, nullptr, EVP_sha256(), nullptr, k) == 1 &&
                  EVP_DigestVerify(md, der, (size_t)dl, (const unsigned char*)msg.data(), msg.size()) == 1;
  EVP_MD_CTX_free(md);
  OPENSSL_free(der);
  ECDSA_SIG_free(es);
  return ok;
}

static std::vector<std::string> messages(size_t n, unsigned seed) {
  std::vector<std::string> m(n);
  for (size_t i = 0; i < n; i++) {
    const size_t len = (i * 37 + seed) % 300;  // 0 .. 299 bytes, the empty message included
    m[i].resize(len);
    for (size_t j = 0; j < len; j++) m[i][j] = (char)((i * 131 + j * 7 + seed) & 0xFF);
  }
  if (n) m[0].clear();
  return m;
}

// signBatch(msgs) as strings
static std::vector<std::string> batch(HipECDSASigner& s, const std::vector<std::string>& msgs) {
  std::vector<std::string> out(msgs.size(), std::string(s.signatureLength(), '\x5A'));
  std::vector<SignRequest> reqs;
  for (size_t i = 0; i < msgs.size(); i++) reqs.push_back({msgs[i].data(), msgs[i].size(), &out[i][0]});
  s.signBatch(reqs);
  return out;
}

static void testK1(bool no_gpu) {
  Key k = makeKey("secp256k1");
  HipECDSASigner hexS(k.hex, KeyFormat::HexaDecimalStrippedFormat), pemS(k.pem, KeyFormat::PemFormat);
  CHECK(hexS.signatureLength() == 64 && pemS.signatureLength() == 64);
  CHECK(hexS.gpuCapable() && pemS.gpuCapable());
  CHECK(hexS.getPrivKey() == k.hex);
  HipECDSAVerifier ver(hexS.getPubKeyHex(), KeyFormat::HexaDecimalStrippedFormat);
  const size_t big = 40, small = 5;
  CHECK(HipECDSASigner::gpuMinBatch() == CBFT_ECDSA_SIGN_GPU_MIN_DEFAULT && small < HipECDSASigner::gpuMinBatch() &&
        big >= HipECDSASigner::gpuMinBatch());
  const auto msgs = messages(big, 3);
  std::vector<std::string> one;
  for (const auto& m : msgs) one.push_back(hexS.sign(m));
  for (size_t i = 0; i < big; i++) {
    CHECK(one[i].size() == 64);
    CHECK(one[i] == pemS.sign(msgs[i]));  // deterministic, and the same key from both encodings
    CHECK(opensslVerify(k.pkey, msgs[i], one[i]));
    CHECK(!opensslVerify(k.pkey, msgs[i] + "x", one[i]));
    CHECK(ver.verify(msgs[i], one[i]));  // a lone verify is below the verifier's GPU threshold: host OpenSSL
  }
  const SignStats s0 = ecdsaSignStats();
  // below gpuMinBatch(): the host loop
  const std::vector<std::string> few(msgs.begin(), msgs.begin() + small);
  const auto hostSigs = batch(hexS, few);
  for (size_t i = 0; i < small; i++) CHECK(hostSigs[i] == one[i]);
  const SignStats s1 = ecdsaSignStats();
  CHECK(s1.host_items == s0.host_items + small && s1.gpu_batches == s0.gpu_batches && s1.gpu_errors == s0.gpu_errors);
  if (no_gpu) return;
  // gpuMinBatch() and more: one GPU call, byte for byte what sign() gives
  const auto gpuSigs = batch(hexS, msgs);
  for (size_t i = 0; i < big; i++) CHECK(gpuSigs[i] == one[i]);
  const auto gpuSigs2 = batch(pemS, msgs);
  for (size_t i = 0; i < big; i++) CHECK(gpuSigs2[i] == one[i]);
  const SignStats s2 = ecdsaSignStats();
  CHECK(s2.gpu_batches == s1.gpu_batches + 2 && s2.gpu_items == s1.gpu_items + 2 * big);
  CHECK(s2.host_items == s1.host_items && s2.gpu_errors == s1.gpu_errors);
  // every GPU signature through the batch verifier
  std::vector<VerifyRequest> vr;
  for (size_t i = 0; i < big; i++) vr.push_back({&ver, msgs[i].data(), msgs[i].size(), gpuSigs[i].data(), 64});
  std::vector<bool> verdicts;
  HipECDSAVerifier::verifyBatch(vr, verdicts);
  for (size_t i = 0; i < big; i++) CHECK(verdicts[i]);
  EVP_PKEY_free(k.pkey);
}

static void testP384() {
  Key k = makeKey("secp384r1");
  HipECDSASigner s(k.pem, KeyFormat::PemFormat), sh(k.hex, KeyFormat::HexaDecimalStrippedFormat);
  CHECK(s.signatureLength() == 96 && !s.gpuCapable() && !sh.gpuCapable());
  HipECDSAVerifier ver(s.getPubKeyHex(), KeyFormat::HexaDecimalStrippedFormat);
  const auto msgs = messages(20, 9);  // above gpuMinBatch(): still the host loop
  const SignStats s0 = ecdsaSignStats();
  const auto sigs = batch(s, msgs);
  const SignStats s1 = ecdsaSignStats();
  CHECK(s1.host_items == s0.host_items + 20 && s1.gpu_batches == s0.gpu_batches && s1.gpu_errors == s0.gpu_errors);
  for (size_t i = 0; i < msgs.size(); i++) {
    CHECK(sigs[i].size() == 96);
    CHECK(opensslVerify(k.pkey, msgs[i], sigs[i]));
    CHECK(ver.verify(msgs[i], sigs[i]));
    CHECK(ver.verify(msgs[i], sh.sign(msgs[i])));
  }
  EVP_PKEY_free(k.pkey);
}

static void testBadKeys() {
  bool threw = false;
  try {
    HipECDSASigner s("00ff", KeyFormat::HexaDecimalStrippedFormat);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {
    HipECDSASigner s("not a pem", KeyFormat::PemFormat);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
}

int main(int argc, char** argv) {
  const bool no_gpu = argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0;
  unsetenv("CBFT_ECDSA_SIGN_GPU_MIN");
  try {
    testBadKeys();
    testK1(no_gpu);
    testP384();
  } catch (const std::exception& e) {
    std::printf("FAIL: exception %s\n", e.what());
    return 1;
  }
  if (g_fail) return 1;
  std::printf(no_gpu ? "all GPU-free checks passed\n" : "all checks passed\n");
  return 0;
}
