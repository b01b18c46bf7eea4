// Host-side test of BLS::Hip::combineBatch: below the crossover (a loop of getFullSignedData), at it and
// above it (one cbft_bls_combine_batch) every out holds the bytes getFullSignedData writes, for
// threshold, n-of-n and k-of-n multisig accumulators; short buffers and an undecodable share give
// ok = false and leave out alone.
//
//   test_bls_combine_host            everything (needs the GPU)
//   test_bls_combine_host --no-gpu   the parts that never open the device: packing, offsets, refusals,
//                                    the crossover setting (the mode a sanitizer build runs on a CPU-only
//                                    machine)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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

static std::vector<uint8_t> records(std::initializer_list<int> ids, uint8_t fill) {
  std::vector<uint8_t> r;
  for (int id : ids) {
    r.insert(r.end(), {0, 0, (uint8_t)(id >> 8), (uint8_t)id});
    r.insert(r.end(), 33, (uint8_t)(fill + id));
  }
  return r;
}

static void testNoGpu() {
  const char* e = std::getenv("CBFT_BLS_COMBINE_BATCH_MIN");
  const long long x = e ? std::atoll(e) : 0;
  CHECK(combineBatchMin() == (x > 0 ? (size_t)x : (size_t)CBFT_BLS_COMBINE_BATCH_MIN_DEFAULT));

  const size_t kTail = 256;
  std::vector<BlsCombineInput> in(8);
  for (auto& a : in) {
    a.usable = true;
    a.multisig = true;
    a.signers.assign(kTail, 0);
  }
  in[0].records = records({1, 2, 3}, 10);
  in[0].signers[0] = 0x07;
  in[1].records = records({2, 5}, 20);  // buffer one byte short
  in[2].records = records({4}, 30);     // no buffer
  in[3].records.clear();                // no valid share: the identity, answered by the plan
  in[3].signers[1] = 0x55;
  in[4].usable = false;                 // not an accumulator of this implementation
  in[5].records = records({1, 2, 3, 4, 5}, 40);
  in[6].records = records({7}, 50);     // negative length
  in[7].records = records({2047, 2048}, 60);
  std::vector<std::vector<char>> buf(8, std::vector<char>(33 + kTail, (char)0xAA));
  std::vector<BlsCombineRequest> r;
  for (size_t i = 0; i < 8; i++) r.push_back({nullptr, buf[i].data(), (int)buf[i].size(), true});
  r[1].outLen = 33 + (int)kTail - 1;
  r[2].out = nullptr;
  r[6].outLen = -1;
  BlsCombinePlan p;
  planCombine(in, r, p);
  CHECK(p.multisig);
  CHECK((p.item == std::vector<uint32_t>{0, 5, 7}));
  CHECK((p.certOff == std::vector<uint64_t>{0, 3, 8, 10}));
  CHECK(p.shares37.size() == 37 * 10);
  CHECK(std::memcmp(p.shares37.data(), in[0].records.data(), 37 * 3) == 0);
  CHECK(std::memcmp(p.shares37.data() + 37 * 3, in[5].records.data(), 37 * 5) == 0);
  CHECK(std::memcmp(p.shares37.data() + 37 * 8, in[7].records.data(), 37 * 2) == 0);
  for (size_t i = 0; i < 8; i++) CHECK(r[i].ok == (i == 3));  // only the identity is answered already
  std::vector<char> ident(33 + kTail, 0);
  ident[33 + 1] = 0x55;
  CHECK(buf[3] == ident);
  for (size_t i : {0, 1, 4, 5, 6, 7}) CHECK(buf[i] == std::vector<char>(33 + kTail, (char)0xAA));  // untouched

  // threshold accumulators: 33 bytes are enough, 32 are not
  std::vector<BlsCombineInput> th(2);
  th[0].usable = th[1].usable = true;
  th[0].records = records({1, 3}, 1);
  th[1].records = records({2, 3}, 2);
  std::vector<BlsCombineRequest> q = {{nullptr, buf[0].data(), 33, true}, {nullptr, buf[1].data(), 32, true}};
  planCombine(th, q, p);
  CHECK(!p.multisig && (p.item == std::vector<uint32_t>{0}) && (p.certOff == std::vector<uint64_t>{0, 2}));
  CHECK(!q[0].ok && !q[1].ok);

  // nothing to do; accumulators of two kinds; an input count that does not match
  std::vector<BlsCombineRequest> none;
  planCombine({}, none, p);
  CHECK(p.item.empty() && p.shares37.empty() && (p.certOff == std::vector<uint64_t>{0}));
  th[1].multisig = true;
  bool threw = false;
  try {
    planCombine(th, q, p);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {
    planCombine(in, q, p);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
}

struct Cert {
  std::unique_ptr<IThresholdAccumulator> acc;
  std::vector<char> want;  // getFullSignedData's bytes; empty: it throws
  int outLen;
};

// combineBatch over the first n certificates, for n around the crossover: every out equals want
static void runSizes(std::vector<Cert>& certs, int fullLen, const char* what) {
  const size_t kMin = combineBatchMin(), total = certs.size();
  for (size_t n : {(size_t)0, (size_t)1, kMin - 1, kMin, kMin + 1, total}) {
    if (n > total) continue;
    std::vector<std::vector<char>> out(n, std::vector<char>((size_t)fullLen, (char)0xAA));
    std::vector<BlsCombineRequest> reqs;
    for (size_t i = 0; i < n; i++) reqs.push_back({certs[i].acc.get(), out[i].data(), certs[i].outLen, certs[i].want.empty()});
    combineBatch(reqs);
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) {
      const bool wantOk = !certs[i].want.empty();
      bad += reqs[i].ok != wantOk;
      bad += out[i] != (wantOk ? certs[i].want : std::vector<char>((size_t)fullLen, (char)0xAA));
    }
    if (bad) std::printf("%s combineBatch(%zu): %zu outputs differ\n", what, n, bad);
    CHECK(bad == 0);
  }
}

static void testCombineBatch() {
  const int kN = 5, kReq = 3;
  const char* skDec[kN] = {"1234567890123456789012345678901234567", "98765432109876543210987654321",
                           "5555555555555555555555555555555555555555", "31415926535897932384626433832795028841",
                           "27182818284590452353602874713526624977"};
  std::vector<std::unique_ptr<BlsThresholdSigner>> signers;
  std::vector<std::string> vk;
  for (int i = 0; i < kN; i++) {
    signers.emplace_back(new BlsThresholdSigner(i + 1, skDec[i]));
    vk.push_back(signers.back()->getShareVerificationKey().toString());
  }
  const size_t total = combineBatchMin() + 20;
  // what an accumulator of verifier v holds for certificate i: `count` shares from signer i on, one of
  // them spoiled (i % 7 == 3: a prefix byte no point has) or none at all (i % 9 == 5)
  auto fill = [&](const BlsThresholdVerifier& v, int count, int fullLen) {
    std::vector<Cert> certs;
    for (size_t i = 0; i < total; i++) {
      Cert c;
      c.acc.reset(v.newAccumulator(false));
      const std::string msg = "sequence number " + std::to_string(i);
      for (int j = 0; j < count && i % 9 != 5; j++) {
        char s[37];
        signers[(i + j) % kN]->signData(msg.data(), (int)msg.size(), s, 37);
        if (i % 7 == 3 && j == 1) s[4] = 5;
        c.acc->add(s, 37);
      }
      c.outLen = i % 8 == 6 ? fullLen - 1 : fullLen;  // every 8th buffer is one byte short
      c.want.assign((size_t)fullLen, (char)0xAA);
      try {
        c.acc->getFullSignedData(c.want.data(), c.outLen);
      } catch (const std::runtime_error&) {
        c.want.clear();
      }
      CHECK(c.want.empty() == (i % 7 == 3 || i % 8 == 6));
      certs.push_back(std::move(c));
    }
    return certs;
  };
  {
    BlsThresholdVerifier v(vk[0], kReq, kN, vk);
    std::vector<Cert> certs = fill(v, kReq, 33);
    runSizes(certs, 33, "threshold");
    // accumulators of two verifiers in one call
    BlsThresholdVerifier v2(vk[1], kReq, kN, vk);
    std::unique_ptr<IThresholdAccumulator> other(v2.newAccumulator(false));
    char o[33];
    std::vector<BlsCombineRequest> reqs = {{certs[0].acc.get(), o, 33, false}, {other.get(), o, 33, false}};
    bool threw = false;
    try {
      combineBatch(reqs);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    CHECK(threw);
    // a null accumulator among good ones
    std::vector<std::vector<char>> out(total, std::vector<char>(33, (char)0xAA));
    reqs.clear();
    for (size_t i = 0; i < total; i++) reqs.push_back({i == 2 ? nullptr : certs[i].acc.get(), out[i].data(), 33, i == 2});
    combineBatch(reqs);
    CHECK(!reqs[2].ok && reqs[0].ok && out[0] == certs[0].want && out[2] == std::vector<char>(33, (char)0xAA));
  }
  {
    BlsMultisigVerifier mv(kN, kN, vk);
    std::vector<Cert> certs = fill(mv, kN, 33);
    runSizes(certs, 33, "multisig n-of-n");
  }
  {
    BlsMultisigVerifier kv(kReq, kN, vk);
    const int len = kv.requiredLengthForSignedData();
    CHECK(len == 33 + 256);
    std::vector<Cert> certs = fill(kv, kReq, len);
    runSizes(certs, len, "multisig k-of-n");
    CHECK(certs[0].want[33] != 0 || certs[0].want[34] != 0);  // the signer bitmap is there
  }
}

int main(int argc, char** argv) {
  const bool noGpu = argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0;
  try {
    testNoGpu();
    if (!noGpu) testCombineBatch();
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
