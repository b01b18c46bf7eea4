// Host-side test of BLS::Hip key generation in the plugin layer: BlsThresholdKeygen, BlsMultisigKeygen and
// BlsThresholdFactory (newRandomSigners, newVerifier, newSigner, newKeyPair) over libcbft_hipcrypto.
//
//   test_bls_keygen_host            everything (needs the GPU)
//   test_bls_keygen_host --no-gpu   the parts that never open the device: the sampling bounds, the decimal
//                                   and hex key encodings, the crossover setting and its environment
//                                   override (the mode a sanitizer build runs on a CPU-only machine)
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "cbft_hipcrypto.h"
#include "threshsign/bls_hip.hpp"

using namespace BLS::Hip;
using Scalar = std::array<uint8_t, 32>;

static int g_fail = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      g_fail++;                                                  \
    }                                                            \
  } while (0)

static const Scalar kR = {0x25, 0x23, 0x64, 0x82, 0x40, 0x00, 0x00, 0x01, 0xba, 0x34, 0x4d, 0x80, 0x00, 0x00, 0x00, 0x07,
                          0xff, 0x9f, 0x80, 0x00, 0x00, 0x00, 0x00, 0x10, 0xa1, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x0d};
static const char* kRDecimal = "16798108731015832284940804142231733909759579603404752749028378864165570215949";

static Scalar small(uint8_t v) {
  Scalar s{};
  s[31] = v;
  return s;
}
static Scalar lcg(uint32_t& st) {  // a scalar below 2^253 < r
  Scalar s;
  for (auto& b : s) b = (uint8_t)((st = st * 1664525u + 1013904223u) >> 24);
  s[0] &= 0x1f;
  return s;
}

static void testNoGpu() {
  const char* e = std::getenv("CBFT_BLS_KEYGEN_BATCH_MIN");
  const long long x = e ? std::atoll(e) : 0;
  CHECK(keygenBatchMin() == (x > 0 ? (size_t)x : (size_t)CBFT_BLS_KEYGEN_BATCH_MIN_DEFAULT));
  CHECK(keygenBatchMin() >= 1);

  // bounds of [1, r)
  Scalar rm1 = kR, rp1 = kR, top{};
  rm1[31] -= 1;
  rp1[31] += 1;
  top.fill(0xff);
  CHECK(!scalarInRange(small(0)) && scalarInRange(small(1)) && scalarInRange(rm1));
  CHECK(!scalarInRange(kR) && !scalarInRange(rp1) && !scalarInRange(top));
  Scalar hi = small(0);
  hi[0] = 0x25;  // 0x25 00 .. 00 < r, 0x26 00 .. 00 > r
  CHECK(scalarInRange(hi));
  hi[0] = 0x26;
  CHECK(!scalarInRange(hi));
  // 2,000 draws: all in range, not all alike, both halves of the range met
  Scalar first{}, s{};
  bool differ = false, low = false, high = false;
  for (int i = 0; i < 2000; i++) {
    sampleScalar(s);
    CHECK(scalarInRange(s));
    if (i == 0) first = s;
    differ = differ || s != first;
    low = low || s[0] < 0x12;
    high = high || s[0] >= 0x13;
  }
  CHECK(differ && low && high);

  // decimal <-> bytes, hex <-> bytes
  CHECK(BlsSecretKey(small(0)).toString() == "0");
  CHECK(BlsSecretKey(small(255)).toString() == "255");
  CHECK(BlsSecretKey(kR).toString() == kRDecimal);
  CHECK(BlsSecretKey(std::string(kRDecimal)).bytes() == kR);
  CHECK(BlsSecretKey(top).toString() ==
        "115792089237316195423570985008687907853269984665640564039457584007913129639935");
  uint32_t st = 99;
  for (int i = 0; i < 50; i++) {
    const Scalar v = lcg(st);
    const BlsSecretKey a(v);
    CHECK(BlsSecretKey(a.toString()).bytes() == v);
    const BlsSecretKey copy = a;
    CHECK(copy.toString() == a.toString() && copy.bytes() == v);
  }
  CHECK(BlsSecretKey().toString().empty());
  std::string hex(130, '0');
  hex[0] = '0';
  hex[1] = '3';
  hex[129] = 'f';
  const BlsPublicKey pk(hex);
  CHECK(pk.toString() == hex && pk.bytes()[0] == 3 && pk.bytes()[64] == 0x0f);
  bool threw = false;
  try {
    BlsPublicKey bad(std::string(129, '0'));
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  // the factory's scheme rule needs no device
  CHECK(BlsThresholdFactory(false).multisigFor(5, 5) && !BlsThresholdFactory(false).multisigFor(3, 5));
  CHECK(BlsThresholdFactory(true).multisigFor(3, 5));
}

// every signer signs, reqSigners shares are accumulated with share verification, the signature verifies;
// another digest does not
static void signAccumulateVerify(const std::vector<IThresholdSigner*>& signers, IThresholdVerifier* v, int k, int n,
                                 const char* what) {
  const std::string digest = "0123456789abcdef0123456789abcdef", other = "0123456789abcdef0123456789abcdeg";
  std::unique_ptr<IThresholdAccumulator> acc(v->newAccumulator(true));
  acc->setExpectedDigest(reinterpret_cast<const unsigned char*>(digest.data()), (int)digest.size());
  CHECK((int)signers.size() == n + 1 && signers[0] == nullptr);
  for (int i = n; i > n - k; i--) {  // the k highest ids
    std::vector<char> share((size_t)signers[(size_t)i]->requiredLengthForSignedData());
    signers[(size_t)i]->signData(digest.data(), (int)digest.size(), share.data(), (int)share.size());
    acc->add(share.data(), (int)share.size());
    CHECK(signers[(size_t)i]->getShareVerificationKey().toString() == v->getShareVerificationKey(i).toString());
  }
  CHECK(acc->getNumValidShares() == k || !acc->hasShareVerificationEnabled());
  std::vector<char> sig((size_t)v->requiredLengthForSignedData());
  acc->getFullSignedData(sig.data(), (int)sig.size());
  const bool good = v->verify(digest.data(), (int)digest.size(), sig.data(), (int)sig.size());
  const bool bad = v->verify(other.data(), (int)other.size(), sig.data(), (int)sig.size());
  if (!good || bad) std::printf("FAIL %s (%d of %d): verify = %d, other digest = %d\n", what, k, n, good, bad);
  CHECK(good && !bad);
}

static void testRandomSigners() {
  const int shapes[4][2] = {{1, 1}, {3, 5}, {5, 5}, {11, 16}};
  for (const auto& kn : shapes) {
    for (const bool multisig : {false, true}) {
      if (multisig && kn[1] != 5) continue;  // the multisig flag: k-of-n (3, 5) and n-of-n (5, 5)
      BlsThresholdFactory f(multisig);
      std::vector<IThresholdSigner*> signers;
      IThresholdVerifier* v = nullptr;
      std::tie(signers, v) = f.newRandomSigners(kn[0], kn[1]);
      std::unique_ptr<IThresholdVerifier> own(v);
      CHECK((dynamic_cast<BlsMultisigVerifier*>(v) != nullptr) == f.multisigFor(kn[0], kn[1]));
      signAccumulateVerify(signers, v, kn[0], kn[1], multisig ? "multisig factory" : "threshold factory");
      // the same keys through their strings: newSigner and newVerifier
      std::vector<std::string> vks(1);
      for (int i = 1; i <= kn[1]; i++) vks.push_back(v->getShareVerificationKey(i).toString());
      std::unique_ptr<IThresholdVerifier> v2(
          f.newVerifier(kn[0], kn[1], v->getPublicKey().toString().c_str(), vks));
      std::vector<IThresholdSigner*> again(signers.size(), nullptr);
      for (int i = 1; i <= kn[1]; i++)
        again[(size_t)i] = f.newSigner(i, signers[(size_t)i]->getShareSecretKey().toString().c_str());
      signAccumulateVerify(again, v2.get(), kn[0], kn[1], "from strings");
      for (auto* s : signers) delete s;
      for (auto* s : again) delete s;
    }
  }
}

static void testInjectedCoefficients() {
  cbft_ctx* ctx = nullptr;
  CHECK(cbft_open(&ctx, 0, 0) == CBFT_OK);
  if (!ctx) return;
  uint32_t st = 7;
  for (const auto& kn : {std::pair<int, int>{1, 1}, {3, 5}, {5, 5}, {11, 16}}) {
    const int k = kn.first, n = kn.second;
    std::vector<Scalar> c((size_t)k);
    for (auto& x : c) x = lcg(st);
    std::vector<uint8_t> sk(32 * (size_t)n), vk(65 * (size_t)n), pk(65), ok((size_t)n + 1);
    CHECK(cbft_bls_keygen_threshold(ctx, c[0].data(), (uint32_t)k, (uint32_t)n, sk.data(), vk.data(), pk.data(),
                                    ok.data()) == CBFT_OK);
    // below, at and above the crossover: the same keys, and those of the C call
    const std::string at = std::to_string(n + 1);
    for (const char* min : {"100000", at.c_str(), "1"}) {
      setenv("CBFT_BLS_KEYGEN_BATCH_MIN", min, 1);
      CHECK(keygenBatchMin() == (size_t)std::atoll(min));
      const BlsThresholdKeygen kg(k, n, c);
      CHECK(kg.getNumSigners() == n && kg.getSecretKey().bytes() == c[0]);
      CHECK(std::memcmp(kg.getPublicKey().bytes().data(), pk.data(), 65) == 0);
      CHECK((int)kg.getShareSecretKeys().size() == n + 1 && (int)kg.getShareVerificationKeys().size() == n + 1);
      for (int i = 1; i <= n; i++) {
        CHECK(std::memcmp(kg.getShareSecretKey(i).bytes().data(), &sk[32 * (size_t)(i - 1)], 32) == 0);
        CHECK(std::memcmp(kg.getShareVerificationKey(i).bytes().data(), &vk[65 * (size_t)(i - 1)], 65) == 0);
      }
    }
    // multisig: the shares are the secrets themselves, PK the key of their sum
    std::vector<Scalar> secrets((size_t)n);
    for (auto& x : secrets) x = lcg(st);
    std::vector<uint8_t> keys(65 * (size_t)n), okb((size_t)n);
    CHECK(cbft_bls_public_key_batch(ctx, secrets[0].data(), (size_t)n, keys.data(), okb.data()) == CBFT_OK);
    std::string pk0;
    for (const char* min : {"100000", at.c_str(), "1"}) {
      setenv("CBFT_BLS_KEYGEN_BATCH_MIN", min, 1);
      const BlsMultisigKeygen mk(n, secrets);
      for (int i = 1; i <= n; i++) {
        CHECK(mk.getShareSecretKey(i).bytes() == secrets[(size_t)i - 1]);
        CHECK(std::memcmp(mk.getShareVerificationKey(i).bytes().data(), &keys[65 * (size_t)(i - 1)], 65) == 0);
      }
      uint8_t sum65[65];
      CHECK(cbft_bls_public_key(ctx, mk.getSecretKey().bytes().data(), sum65) == CBFT_OK);
      CHECK(std::memcmp(mk.getPublicKey().bytes().data(), sum65, 65) == 0);
      if (pk0.empty()) pk0 = mk.getPublicKey().toString();
      CHECK(mk.getPublicKey().toString() == pk0);
      if (n == 1) CHECK(mk.getSecretKey().bytes() == secrets[0]);
    }
    unsetenv("CBFT_BLS_KEYGEN_BATCH_MIN");
  }
  // a share that is 0 mod r is refused: c_0 = r - 3, c_1 = 1 gives f(3) = 0
  {
    Scalar c0 = kR;
    c0[31] -= 3;
    bool threw = false;
    try {
      BlsThresholdKeygen kg(2, 5, {c0, small(1)});
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
      BlsThresholdKeygen kg(3, 2);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    CHECK(threw);
  }
  cbft_close(ctx);
}

static void testKeyPair() {
  BlsThresholdFactory f(true);
  auto kp = f.newKeyPair();
  CHECK(kp.first && kp.second && kp.second->toString().size() == 130);
  std::vector<IThresholdSigner*> signers(2, nullptr);
  signers[1] = f.newSigner(1, kp.first->toString().c_str());
  CHECK(signers[1]->getShareVerificationKey().toString() == kp.second->toString());
  std::unique_ptr<IThresholdVerifier> v(f.newVerifier(1, 1, "", {std::string(), kp.second->toString()}));
  signAccumulateVerify(signers, v.get(), 1, 1, "newKeyPair");
  delete signers[1];
  auto kp2 = f.newKeyPair();
  CHECK(kp2.first->toString() != kp.first->toString());
  bool threw = false;
  try {
    BlsThresholdFactory(false).newKeyPair();
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
}

int main(int argc, char** argv) {
  const bool noGpu = argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0;
  try {
    testNoGpu();
    if (!noGpu) {
      testRandomSigners();
      testInjectedCoefficients();
      testKeyPair();
    }
  } catch (const std::exception& e) {
    std::printf("FAIL: exception: %s\n", e.what());
    return 1;
  }
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf(noGpu ? "all GPU-free checks passed\n" : "all checks passed\n");
  return 0;
}
