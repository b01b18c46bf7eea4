// C++ host-side tests of batched signing in the plugin layer (run on the GPU box by
// tests/test_cpp_sign_host.py): EdDSASigner::signBatch on both sides of its crossover,
// HipSigManager::signBatch with an Ed25519 and with an RSA own key, signPreProcessReplyHashes
// verified back through verifySigBatch, and the host fall-back when the GPU engine cannot open.
#include <openssl/bn.h>
#include <openssl/evp.h>
#include <openssl/rsa.h>
#include <openssl/x509.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <set>
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

static std::string seedHex(int i) {
  std::mt19937 g(7000 + i);
  uint8_t b[32];
  for (auto& x : b) x = (uint8_t)g();
  return toHex(b, 32);
}

static std::vector<std::string> messages(size_t n, int salt) {
  std::mt19937 g(salt);
  std::vector<std::string> m(n);
  for (size_t i = 0; i < n; i++) {
    m[i].resize(i % 7 == 0 ? 32 : g() % 300);  // empty ones too
    for (auto& c : m[i]) c = (char)g();
  }
  return m;
}

// signBatch(msgs) == sign(msg) item by item
static int batchEqualsSign(EdDSASigner& s, const std::vector<std::string>& msgs) {
  std::vector<char> out(msgs.size() * 64, '\x5a');
  std::vector<SignRequest> reqs;
  for (size_t i = 0; i < msgs.size(); i++) reqs.push_back({msgs[i].data(), msgs[i].size(), &out[64 * i]});
  s.signBatch(reqs);
  for (size_t i = 0; i < msgs.size(); i++) CHECK(s.sign(msgs[i]) == std::string(&out[64 * i], 64));
  return 0;
}

static std::string genRsaPrivHex(std::string* pubHex) {
  EVP_PKEY_CTX* c = EVP_PKEY_CTX_new_id(EVP_PKEY_RSA, nullptr);
  EVP_PKEY* k = nullptr;
  BIGNUM* be = BN_new();
  BN_set_word(be, 17);
  EVP_PKEY_keygen_init(c);
  EVP_PKEY_CTX_set_rsa_keygen_bits(c, 2048);
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

// The engine cannot open (no such device): signBatch above the crossover still signs, on the
// host, and the failure is counted.  Runs first, before anything opened the engine.
static int testForcedGpuFailure() {
  setEd25519Device(9999);
  EdDSASigner s(seedHex(1), KeyFormat::HexaDecimalStrippedFormat);
  const size_t n = EdDSASigner::gpuMinBatch() * 2;
  const SignStats a = ed25519SignStats();
  CHECK(batchEqualsSign(s, messages(n, 1)) == 0);
  const SignStats b = ed25519SignStats();
  CHECK(b.gpu_errors == a.gpu_errors + 1);
  CHECK(b.gpu_batches == a.gpu_batches && b.host_items == a.host_items + n);
  setEd25519Device(0);
  return 0;
}

static int testSignerBatch() {
  const size_t min = EdDSASigner::gpuMinBatch();
  CHECK(min >= 2);
  EdDSASigner s(seedHex(2), KeyFormat::HexaDecimalStrippedFormat);
  SignStats a = ed25519SignStats();
  CHECK(batchEqualsSign(s, messages(min - 1, 2)) == 0);  // below the crossover: host loop
  SignStats b = ed25519SignStats();
  CHECK(b.gpu_batches == a.gpu_batches && b.host_items == a.host_items + min - 1 && b.gpu_errors == a.gpu_errors);
  for (size_t n : {min, min + 1, (size_t)1000}) {  // at and above it: one GPU batch each
    a = ed25519SignStats();
    CHECK(batchEqualsSign(s, messages(n, (int)n)) == 0);
    b = ed25519SignStats();
    CHECK(b.gpu_batches == a.gpu_batches + 1 && b.gpu_items == a.gpu_items + n);
    CHECK(b.host_items == a.host_items && b.gpu_errors == a.gpu_errors);
  }
  s.signBatch({});  // nothing to do
  // a moved signer keeps signing (its registration moves with it); a second signer has its own key
  EdDSASigner moved(std::move(s));
  EdDSASigner other(seedHex(3), KeyFormat::HexaDecimalStrippedFormat);
  CHECK(batchEqualsSign(moved, messages(min + 5, 11)) == 0);
  CHECK(batchEqualsSign(other, messages(min + 5, 11)) == 0);
  return 0;
}

static int testSigManager() {
  ReplicaIdsConfig cfg;
  cfg.replicaId = 0;
  cfg.numOfExternalClients = 2;
  ReplicasInfo ri(cfg);
  // --- Ed25519 own key: signBatch == sign, and signPreProcessReplyHashes verifies for our own id
  std::vector<EdDSASigner> rs;
  HipSigManager::ReplicaKeys replicaKeys;
  for (int r = 0; r < 4; r++) {
    rs.emplace_back(seedHex(100 + r), KeyFormat::HexaDecimalStrippedFormat);
    replicaKeys.insert({(PrincipalId)r, rs.back().getPubKeyHex()});
  }
  std::unique_ptr<HipSigManager> sm(HipSigManager::initInTesting(
      0, seedHex(100), replicaKeys, KeyFormat::HexaDecimalStrippedFormat, nullptr, KeyFormat::HexaDecimalStrippedFormat, ri));
  CHECK(sm->getMySigLength() == 64);
  const size_t n = EdDSASigner::gpuMinBatch() * 4 + 3;
  std::vector<std::string> msgs = messages(n, 21);
  std::vector<char> out(n * 64);
  std::vector<SignRequest> reqs;
  for (size_t i = 0; i < n; i++) reqs.push_back({msgs[i].data(), msgs[i].size(), &out[64 * i]});
  const SignStats a = ed25519SignStats();
  sm->signBatch(reqs);
  const SignStats b = ed25519SignStats();
  CHECK(b.gpu_batches == a.gpu_batches + 1 && b.gpu_errors == a.gpu_errors);
  for (size_t i = 0; i < n; i++) {
    char one[64];
    sm->sign(msgs[i].data(), msgs[i].size(), one, 64);
    CHECK(std::memcmp(one, &out[64 * i], 64) == 0);
  }
  CHECK(recorders().sig_manager_sign_batch.count() >= 1);

  std::vector<uint8_t> hashes(n * 32);
  for (size_t i = 0; i < n; i++) {
    const std::string h = preProcessResultHash(msgs[i].data(), (uint32_t)msgs[i].size(), 0, 4, 1000 + i);
    CHECK(h.size() == 32);
    std::memcpy(&hashes[32 * i], h.data(), 32);
  }
  std::vector<char> sigs(n * 64);
  signPreProcessReplyHashes(*sm, hashes.data(), n, sigs.data());
  std::vector<SigBatchItem> items;
  for (size_t i = 0; i < n; i++)
    items.push_back({0, reinterpret_cast<const char*>(&hashes[32 * i]), 32, &sigs[64 * i], 64});
  std::vector<bool> ok;
  CHECK(sm->verifySigBatch(items, ok) == n);
  for (size_t i = 0; i < n; i++) CHECK(ok[i]);
  hashes[32 * 5 + 1] ^= 1;  // a changed hash no longer verifies under its signature
  CHECK(sm->verifySigBatch(items, ok) == 5 && !ok[5] && ok[4] && ok[6]);

  // --- RSA own key: the host loop over SigManager::sign (deterministic PKCS#1 v1.5)
  std::string rsaPub;
  const std::string rsaPriv = genRsaPrivHex(&rsaPub);
  HipSigManager::ReplicaKeys rsaKeys;
  for (int r = 0; r < 4; r++) rsaKeys.insert({(PrincipalId)r, rsaPub});
  std::unique_ptr<HipSigManager> smr(HipSigManager::initInTesting(
      0, rsaPriv, rsaKeys, KeyFormat::HexaDecimalStrippedFormat, nullptr, KeyFormat::HexaDecimalStrippedFormat, ri));
  CHECK(smr->getMySigLength() == 256);
  const size_t m = 5;
  std::vector<char> rout(m * 256), rone(256);
  std::vector<SignRequest> rreqs;
  for (size_t i = 0; i < m; i++) rreqs.push_back({msgs[i].data(), msgs[i].size(), &rout[256 * i]});
  const SignStats c = ed25519SignStats();
  smr->signBatch(rreqs);
  const SignStats d = ed25519SignStats();
  CHECK(d.gpu_batches == c.gpu_batches && d.host_items == c.host_items);  // not an Ed25519 batch at all
  std::vector<SigBatchItem> ritems;
  for (size_t i = 0; i < m; i++) {
    smr->sign(msgs[i].data(), msgs[i].size(), rone.data(), 256);
    CHECK(std::memcmp(rone.data(), &rout[256 * i], 256) == 0);
    ritems.push_back({0, msgs[i].data(), msgs[i].size(), &rout[256 * i], 256});
  }
  CHECK(smr->verifySigBatch(ritems, ok) == m);
  std::vector<uint8_t> h2(3 * 32, 7);
  std::vector<char> s2(3 * 256);
  signPreProcessReplyHashes(*smr, h2.data(), 3, s2.data());
  smr->sign(reinterpret_cast<const char*>(h2.data()), 32, rone.data(), 256);
  CHECK(std::memcmp(rone.data(), &s2[256 * 2], 256) == 0);
  return 0;
}

int main() {
  if (testForcedGpuFailure()) return 1;
  if (testSignerBatch()) return 1;
  if (testSigManager()) return 1;
  std::printf("test_sign_host: all checks passed\n");
  return 0;
}
