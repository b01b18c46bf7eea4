// Host-side test of BLS::Hip::BlsThresholdSigner::signBatch: below the crossover (a loop of
// cbft_bls_sign), at it and above it (one cbft_bls_sign_batch) the bytes are those of signData.
//
//   test_bls_sign_host            everything (needs the GPU)
//   test_bls_sign_host --no-gpu   the parts that never open the device: key parsing, the crossover
//                                 setting (the mode the sanitizer build runs on a CPU-only machine)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "threshsign/bls_hip.hpp"

using namespace BLS::Hip;

static int g_fail = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      g_fail++;                                                  \
    }                                                            \
  } while (0)

// a share secret key below r, in decimal (BlsSecretKey's encoding)
static const char* kSkDec = "7934650183025465912345678901234567890123456789012345678901234567890123";

template <class E, class F>
static bool throws(F f) {
  try {
    f();
  } catch (const E&) {
    return true;
  } catch (...) {
  }
  return false;
}

static void testNoGpu() {
  BlsSecretKey one("1"), big(kSkDec);
  CHECK(one.bytes()[31] == 1 && one.bytes()[0] == 0);
  CHECK(big.toString() == kSkDec);
  // 256 = 0x0100
  BlsSecretKey k256("256");
  CHECK(k256.bytes()[30] == 1 && k256.bytes()[31] == 0);
  CHECK(throws<std::invalid_argument>([] { BlsSecretKey bad("12x4"); }));
  CHECK(throws<std::invalid_argument>([] { BlsSecretKey bad(""); }));
  CHECK(throws<std::invalid_argument>([] { BlsPublicKey bad("abcd"); }));
  CHECK(throws<std::invalid_argument>([] { BlsPublicKey bad(std::string(130, 'g')); }));
  BlsPublicKey pk(std::string(130, 'a'));
  CHECK(pk.bytes()[0] == 0xaa && pk.bytes()[64] == 0xaa);
  const char* e = std::getenv("CBFT_BLS_SIGN_BATCH_MIN");
  const long long x = e ? std::atoll(e) : 0;
  CHECK(BlsThresholdSigner::batchMin() == (x > 0 ? (size_t)x : (size_t)CBFT_BLS_SIGN_BATCH_MIN_DEFAULT));
}

static void testSignBatch() {
  BlsThresholdSigner signer(5, kSkDec);
  const size_t kMin = BlsThresholdSigner::batchMin();
  const size_t total = kMin + 40;
  // messages: 32-byte digests, and a few other lengths (0, 1, 100 bytes)
  std::vector<std::string> msgs(total);
  uint32_t st = 12345;
  for (size_t i = 0; i < total; i++) {
    const size_t len = i == 1 ? 0 : i == 2 ? 1 : i == 3 ? 100 : 32;
    msgs[i].resize(len);
    for (auto& c : msgs[i]) c = (char)((st = st * 1664525u + 1013904223u) >> 24);
  }
  std::vector<std::vector<char>> ref(total, std::vector<char>(37));
  for (size_t i = 0; i < total; i++) signer.signData(msgs[i].data(), (int)msgs[i].size(), ref[i].data(), 37);
  CHECK((uint8_t)ref[0][3] == 5 && ref[0][0] == 0);

  for (size_t n : {(size_t)0, (size_t)1, kMin - 1, kMin, kMin + 1, total}) {
    if (n > total) continue;
    std::vector<std::vector<char>> out(n, std::vector<char>(40, (char)0x5a));
    std::vector<BlsSignRequest> reqs;
    for (size_t i = 0; i < n; i++) reqs.push_back({msgs[i].data(), (int)msgs[i].size(), out[i].data(), 40});
    signer.signBatch(reqs);
    size_t bad = 0;
    for (size_t i = 0; i < n; i++)
      if (std::memcmp(out[i].data(), ref[i].data(), 37) != 0 || out[i][37] != (char)0x5a) bad++;
    if (bad) std::printf("signBatch(%zu): %zu shares differ from signData\n", n, bad);
    CHECK(bad == 0);
  }

  // a short output buffer anywhere in the batch: refused before anything is signed
  std::vector<std::vector<char>> out(total, std::vector<char>(37, (char)0x5a));
  std::vector<BlsSignRequest> reqs;
  for (size_t i = 0; i < total; i++) reqs.push_back({msgs[i].data(), (int)msgs[i].size(), out[i].data(), 37});
  reqs[total - 1].outLen = 36;
  CHECK(throws<std::runtime_error>([&] { signer.signBatch(reqs); }));
  CHECK(out[0][0] == (char)0x5a && out[total - 2][36] == (char)0x5a);
  reqs[total - 1].outLen = 37;
  reqs[0].hash = nullptr;
  CHECK(throws<std::invalid_argument>([&] { signer.signBatch(reqs); }));

  // two signers, each with its own table
  BlsThresholdSigner other(2048, "12345678901234567890");
  std::vector<char> a(37), b(37);
  other.signData(msgs[0].data(), 32, a.data(), 37);
  std::vector<std::vector<char>> o2(kMin, std::vector<char>(37));
  std::vector<BlsSignRequest> r2;
  for (size_t i = 0; i < kMin; i++) r2.push_back({msgs[0].data(), 32, o2[i].data(), 37});
  other.signBatch(r2);
  CHECK(std::memcmp(o2[kMin - 1].data(), a.data(), 37) == 0);
  CHECK(std::memcmp(a.data(), ref[0].data(), 37) != 0);
}

int main(int argc, char** argv) {
  const bool noGpu = argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0;
  try {
    testNoGpu();
    if (!noGpu) testSignBatch();
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
