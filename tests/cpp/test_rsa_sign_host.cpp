// C++ host-side tests of batched RSA signing in the plugin layer (run on the GPU box by
// tests/test_cpp_rsa_sign_host.py): HipRSASigner::signBatch on both sides of its crossover,
// HipSigManager::signBatch and signPreProcessReplyHashes with an RSA own key on the GPU, the host
// fall-back when the GPU engine cannot open, and a 3,072-bit key that never leaves the host.
#include <openssl/bn.h>
#include <openssl/evp.h>
#include <openssl/rsa.h>
#include <openssl/x509.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "ReplicaConfig.hpp"
#include "hip_crypto.hpp"
#include "hip_sig_manager.hpp"
#include "request_batch.hpp"

using namespace concord::hip;
using bftEngine::impl::PrincipalId;
using bftEngine::impl::ReplicaIdsConfig;
using bftEngine::impl::ReplicasInfo;
using concord::util::crypto::KeyFormat;

#define CHECK(c)                                                                \
  do {                                                                          \
    if (!(c)) {                                                                 \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

static std::vector<std::string> messages(size_t n, int salt) {
  std::mt19937 g(salt);
  std::vector<std::string> m(n);
  for (size_t i = 0; i < n; i++) {
    m[i].resize(i % 7 == 0 ? 32 : g() % 300);  // empty ones too
    for (auto& c : m[i]) c = (char)g();
  }
  return m;
}

static std::string genRsaPrivHex(int bits, unsigned long e, std::string* pubHex) {
  EVP_PKEY_CTX* c = EVP_PKEY_CTX_new_id(EVP_PKEY_RSA, nullptr);
  EVP_PKEY* k = nullptr;
  BIGNUM* be = BN_new();
  BN_set_word(be, e);
  EVP_PKEY_keygen_init(c);
  EVP_PKEY_CTX_set_rsa_keygen_bits(c, bits);
  EVP_PKEY_CTX_set1_rsa_keygen_pubexp(c, be);
  EVP_PKEY_keygen(c, &k);
  unsigned char* der = nullptr;
  int n = i2d_PrivateKey(k, &der);
  std::string priv = toHex(der, n);
  OPENSSL_free(der);
  der = nullptr;
  n = i2d_PUBKEY(k, &der);
  *pubHex = toHex(der, n);
  OPENSSL_free(der);
  BN_free(be);
  EVP_PKEY_free(k);
  EVP_PKEY_CTX_free(c);
  return priv;
}

// signBatch(msgs) == sign(msg) item by item
static int batchEqualsSign(HipRSASigner& s, const std::vector<std::string>& msgs) {
  const size_t sl = s.signatureLength();
  std::vector<char> out(msgs.size() * sl, '\x5a');
  std::vector<SignRequest> reqs;
  for (size_t i = 0; i < msgs.size(); i++) reqs.push_back({msgs[i].data(), msgs[i].size(), &out[sl * i]});
  s.signBatch(reqs);
  for (size_t i = 0; i < msgs.size(); i++) CHECK(s.sign(msgs[i]) == std::string(&out[sl * i], sl));
  return 0;
}

// The engine cannot open (no such device): signBatch above the crossover still signs, on the
// host, and the failure is counted.  Runs first, before anything opened the engine.
static int testForcedGpuFailure(const std::string& priv) {
  setenv("CBFT_DEVICE", "9999", 1);
  HipRSASigner s(priv, KeyFormat::HexaDecimalStrippedFormat);
  CHECK(s.gpuCapable());
  const size_t n = HipRSASigner::gpuMinBatch() + 2;
  const SignStats a = rsaSignStats();
  CHECK(batchEqualsSign(s, messages(n, 1)) == 0);
  const SignStats b = rsaSignStats();
  CHECK(b.gpu_errors == a.gpu_errors + 1);
  CHECK(b.gpu_batches == a.gpu_batches && b.host_items == a.host_items + n);
  unsetenv("CBFT_DEVICE");
  // the same signer reaches the GPU once an engine can open
  CHECK(batchEqualsSign(s, messages(n, 2)) == 0);
  const SignStats c = rsaSignStats();
  CHECK(c.gpu_batches == b.gpu_batches + 1 && c.gpu_items == b.gpu_items + n && c.gpu_errors == b.gpu_errors);
  return 0;
}

static int testSignerBatch(const std::string& priv, const std::string& priv65537) {
  const size_t min = HipRSASigner::gpuMinBatch();
  CHECK(min >= 2);
  HipRSASigner s(priv, KeyFormat::HexaDecimalStrippedFormat);
  CHECK(s.signatureLength() == 256 && s.getPrivKey() == priv);
  SignStats a = rsaSignStats();
  CHECK(batchEqualsSign(s, messages(min - 1, 3)) == 0);  // below the crossover: host loop
  SignStats b = rsaSignStats();
  CHECK(b.gpu_batches == a.gpu_batches && b.host_items == a.host_items + min - 1 && b.gpu_errors == a.gpu_errors);
  for (size_t n : {min, min + 1, 2 * min + 3}) {  // at and above it: one GPU batch each
    a = rsaSignStats();
    CHECK(batchEqualsSign(s, messages(n, (int)n)) == 0);
    b = rsaSignStats();
    CHECK(b.gpu_batches == a.gpu_batches + 1 && b.gpu_items == a.gpu_items + n);
    CHECK(b.host_items == a.host_items && b.gpu_errors == a.gpu_errors);
  }
  s.signBatch({});  // nothing to do
  // a second signer has its own key and table; makeSigner gives the batch signer for an RSA key
  std::unique_ptr<ISigner> made = makeSigner(priv65537, KeyFormat::HexaDecimalStrippedFormat);
  auto* other = dynamic_cast<HipRSASigner*>(made.get());
  CHECK(other != nullptr);
  CHECK(dynamic_cast<concord::util::crypto::RSASigner*>(made.get()) != nullptr);
  CHECK(batchEqualsSign(*other, messages(min + 5, 11)) == 0);
  CHECK(batchEqualsSign(s, messages(min + 5, 11)) == 0);
  return 0;
}

static int testSigManager(const std::string& priv, const std::string& pub) {
  ReplicaIdsConfig cfg;
  cfg.replicaId = 0;
  cfg.numOfExternalClients = 2;
  ReplicasInfo ri(cfg);
  HipSigManager::ReplicaKeys keys;
  for (int r = 0; r < 4; r++) keys.insert({(PrincipalId)r, pub});
  std::unique_ptr<HipSigManager> sm(HipSigManager::initInTesting(
      0, priv, keys, KeyFormat::HexaDecimalStrippedFormat, nullptr, KeyFormat::HexaDecimalStrippedFormat, ri));
  CHECK(sm->getMySigLength() == 256);
  const size_t n = HipRSASigner::gpuMinBatch() * 2 + 3;
  std::vector<std::string> msgs = messages(n, 21);
  std::vector<char> out(n * 256), one(256);
  std::vector<SignRequest> reqs;
  for (size_t i = 0; i < n; i++) reqs.push_back({msgs[i].data(), msgs[i].size(), &out[256 * i]});
  const SignStats a = rsaSignStats();
  sm->signBatch(reqs);
  const SignStats b = rsaSignStats();
  CHECK(b.gpu_batches == a.gpu_batches + 1 && b.gpu_items == a.gpu_items + n && b.gpu_errors == a.gpu_errors);
  for (size_t i = 0; i < n; i++) {
    sm->sign(msgs[i].data(), msgs[i].size(), one.data(), 256);
    CHECK(std::memcmp(one.data(), &out[256 * i], 256) == 0);
  }
  // the pre-processing path: one signature per result hash, on the GPU, verified back
  std::vector<uint8_t> hashes(n * 32);
  for (size_t i = 0; i < n; i++) {
    const std::string h = preProcessResultHash(msgs[i].data(), (uint32_t)msgs[i].size(), 0, 4, 1000 + i);
    CHECK(h.size() == 32);
    std::memcpy(&hashes[32 * i], h.data(), 32);
  }
  std::vector<char> sigs(n * 256);
  signPreProcessReplyHashes(*sm, hashes.data(), n, sigs.data());
  const SignStats c = rsaSignStats();
  CHECK(c.gpu_batches == b.gpu_batches + 1 && c.gpu_errors == b.gpu_errors);
  std::vector<SigBatchItem> items;
  for (size_t i = 0; i < n; i++)
    items.push_back({0, reinterpret_cast<const char*>(&hashes[32 * i]), 32, &sigs[256 * i], 256});
  std::vector<bool> ok;
  CHECK(sm->verifySigBatch(items, ok) == n);
  sm->sign(reinterpret_cast<const char*>(&hashes[32 * 2]), 32, one.data(), 256);
  CHECK(std::memcmp(one.data(), &sigs[256 * 2], 256) == 0);
  hashes[32 * 5 + 1] ^= 1;  // a changed hash no longer verifies under its signature
  CHECK(sm->verifySigBatch(items, ok) == 5 && !ok[5] && ok[4] && ok[6]);
  return 0;
}

// a 3,072-bit key signs on the host only, whatever the batch size
static int testLargeKeyStaysOnHost() {
  std::string pub;
  const std::string priv = genRsaPrivHex(3072, 65537, &pub);
  HipRSASigner s(priv, KeyFormat::HexaDecimalStrippedFormat);
  CHECK(!s.gpuCapable() && s.signatureLength() == 384);
  const size_t n = HipRSASigner::gpuMinBatch() + 1;
  const SignStats a = rsaSignStats();
  CHECK(batchEqualsSign(s, messages(n, 31)) == 0);
  const SignStats b = rsaSignStats();
  CHECK(b.gpu_batches == a.gpu_batches && b.gpu_errors == a.gpu_errors && b.host_items == a.host_items + n);
  return 0;
}

int main() {
  std::string pub17, pub65537;
  const std::string priv17 = genRsaPrivHex(2048, 17, &pub17);
  const std::string priv65537 = genRsaPrivHex(2048, 65537, &pub65537);
  if (testForcedGpuFailure(priv17)) return 1;
  if (testSignerBatch(priv17, priv65537)) return 1;
  if (testSigManager(priv17, pub17)) return 1;
  if (testLargeKeyStaysOnHost()) return 1;
  std::printf("test_rsa_sign_host: all checks passed\n");
  return 0;
}
