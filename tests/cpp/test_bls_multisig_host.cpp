// Host-side test of BLS::Hip::BlsMultisigVerifier::verifyBatch for k-of-n keys: below the crossover (a
// loop of verify()), at it and above it (one cbft_bls_verify_multisig_batch) the verdicts are those of
// verify() item by item, for certificates mixed with share requests, wrong-length entries, too few
// signers, an id above numSigners, duplicate bitmaps and duplicate digests.
//
//   test_bls_multisig_host            everything (needs the GPU)
//   test_bls_multisig_host --no-gpu   the parts that never open the device: request validation, bitmap
//                                     and digest deduplication, the crossover setting and its environment
//                                     override (the mode a sanitizer build runs on a CPU-only machine)
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

static const size_t kSet = 256, kCert = 33 + kSet;

static std::vector<std::string> makeMsgs(size_t count) {
  std::vector<std::string> msgs(count);
  uint32_t st = 2525;
  for (size_t i = 0; i < count; i++) {
    const size_t len = i == 1 ? 0 : i == 2 ? 1 : i == 3 ? 100 : 32;
    msgs[i].resize(len);
    for (auto& c : msgs[i]) c = (char)((st = st * 1664525u + 1013904223u) >> 24);
  }
  return msgs;
}

// sigma33 (filled with `fill`) || the bitmap of ids
static std::vector<char> makeCert(char fill, std::initializer_list<int> ids) {
  std::vector<char> c(kCert, 0);
  for (size_t i = 0; i < 33; i++) c[i] = (char)(fill + i);
  for (int id : ids) c[33 + (id - 1) / 8] |= (char)(1 << ((id - 1) % 8));
  return c;
}

static void testNoGpu() {
  const char* e = std::getenv("CBFT_BLS_MULTISIG_BATCH_MIN");
  const long long x = e ? std::atoll(e) : 0;
  CHECK(BlsMultisigVerifier::multisigBatchMin() == (x > 0 ? (size_t)x : (size_t)CBFT_BLS_MULTISIG_BATCH_MIN_DEFAULT));
  CHECK(BlsMultisigVerifier::multisigBatchMin() >= 1);
  CHECK(VectorOfShares::getByteCount() == (int)kSet);

  std::vector<std::string> msgs = makeMsgs(6);
  const std::string dup = msgs[4];  // equal bytes at another address
  // 3-of-5
  std::vector<char> a = makeCert(1, {1, 2, 3}), b = makeCert(50, {2, 4, 5}), a2 = makeCert(90, {1, 2, 3}),
                    few = makeCert(1, {1, 2}), above = makeCert(1, {1, 2, 3, 6}), far = makeCert(1, {1, 2, 3, 2048}),
                    all = makeCert(7, {1, 2, 3, 4, 5}), share(37, 9);
  std::vector<BlsVerifyRequest> r = {
      {msgs[0].data(), 32, a.data(), (int)kCert, 0, true},       // 0: certificate, set {1,2,3}
      {msgs[4].data(), 32, b.data(), (int)kCert, 0, true},       // 1: another set, another digest
      {dup.data(), 32, a2.data(), (int)kCert, 0, true},          // 2: set of 0 again, digest of 1 again
      {msgs[0].data(), 32, share.data(), 37, 2, true},           // 3: a share request: left alone
      {msgs[0].data(), 32, a.data(), 33, 0, true},               // 4: the signature without its bitmap
      {msgs[0].data(), 32, a.data(), (int)kCert - 1, 0, true},   // 5: one byte short
      {msgs[0].data(), 32, few.data(), (int)kCert, 0, true},     // 6: too few signers
      {msgs[0].data(), 32, above.data(), (int)kCert, 0, true},   // 7: id 6 > numSigners
      {msgs[0].data(), 32, far.data(), (int)kCert, 0, true},     // 8: id 2048 > numSigners
      {nullptr, 32, a.data(), (int)kCert, 0, true},              // 9
      {msgs[0].data(), -1, a.data(), (int)kCert, 0, true},       // 10
      {msgs[0].data(), 32, nullptr, (int)kCert, 0, true},        // 11
      {msgs[1].data(), 0, all.data(), (int)kCert, 0, true},      // 12: the empty message, every signer
      {msgs[3].data(), 100, b.data(), (int)kCert, 0, true},      // 13: a long message, set of 1 again
      {msgs[0].data(), 32, b.data(), (int)kCert, 0, true},       // 14: digest of 0 under the set of 1
  };
  BlsMultisigPlan p;
  BlsMultisigVerifier::planMultisigBatch(r, 3, 5, p);
  const std::vector<uint32_t> item = {0, 1, 2, 12, 13, 14}, sof = {0, 1, 0, 2, 1, 1}, mof = {0, 1, 1, 2, 3, 0},
                              len = {32, 32, 0, 100};
  const std::vector<uint64_t> off = {0, 32, 64, 64};
  CHECK(p.item == item && p.setOf == sof && p.msgOf == mof && p.msgLen == len && p.msgOff == off);
  CHECK(p.blob.size() == 164 && p.sig33.size() == 33 * item.size() && p.sets.size() == 3 * kSet);
  CHECK(std::memcmp(p.blob.data(), msgs[0].data(), 32) == 0 && std::memcmp(p.blob.data() + 32, msgs[4].data(), 32) == 0);
  CHECK(std::memcmp(p.blob.data() + 64, msgs[3].data(), 100) == 0);
  CHECK(std::memcmp(&p.sets[0], a.data() + 33, kSet) == 0 && std::memcmp(&p.sets[kSet], b.data() + 33, kSet) == 0);
  CHECK(std::memcmp(&p.sets[2 * kSet], all.data() + 33, kSet) == 0);
  CHECK(std::memcmp(&p.sig33[0], a.data(), 33) == 0 && std::memcmp(&p.sig33[66], a2.data(), 33) == 0);
  for (size_t i = 0; i < r.size(); i++) CHECK(r[i].ok == (i == 3));  // certificates start false; the share is untouched
  // every signer required but one: a set of all five still passes, four do not
  std::vector<BlsVerifyRequest> q = {{msgs[0].data(), 32, all.data(), (int)kCert, 0, true},
                                     {msgs[0].data(), 32, b.data(), (int)kCert, 0, true}};
  BlsMultisigVerifier::planMultisigBatch(q, 5, 6, p);
  CHECK(p.item == std::vector<uint32_t>{0} && p.sets.size() == kSet);
  std::vector<BlsVerifyRequest> none;
  BlsMultisigVerifier::planMultisigBatch(none, 3, 5, p);
  CHECK(p.item.empty() && p.blob.empty() && p.sets.empty());
}

struct Ref {
  std::string msg;
  std::vector<char> sig;
  ShareID signer;
  bool want;
};

static void runSizes(const BlsMultisigVerifier& v, const std::vector<Ref>& ref, const char* what) {
  const size_t kMin = BlsMultisigVerifier::multisigBatchMin(), total = ref.size();
  // every third reference is a share or an entry the plan refuses: 3 n entries hold about 2 n certificates
  for (size_t n : {(size_t)0, (size_t)1, kMin - 1, kMin, kMin + 1, 2 * kMin, total}) {
    if (n > total) continue;
    std::vector<BlsVerifyRequest> reqs;
    for (size_t i = 0; i < n; i++)
      reqs.push_back({ref[i].msg.data(), (int)ref[i].msg.size(), ref[i].sig.data(), (int)ref[i].sig.size(),
                      ref[i].signer, !ref[i].want});
    v.verifyBatch(reqs);
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) bad += reqs[i].ok != ref[i].want;
    if (bad) std::printf("%s verifyBatch(%zu): %zu verdicts differ\n", what, n, bad);
    CHECK(bad == 0);
  }
}

static void testVerifyBatch() {
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
  BlsMultisigVerifier kv(kReq, kN, vk);
  const int len = kv.requiredLengthForSignedData();
  CHECK(len == (int)kCert);
  const size_t kMin = BlsMultisigVerifier::multisigBatchMin(), total = 3 * kMin + 40;
  std::vector<std::string> msgs = makeMsgs(9);  // few digests and few signer sets, many entries
  msgs.erase(msgs.begin() + 1);                 // (an accumulator takes no empty digest)
  std::vector<Ref> ref;
  size_t valid = 0, certs = 0;
  for (size_t i = 0; i < total; i++) {
    const std::string& m = msgs[i % msgs.size()];
    Ref r;
    r.msg = m;
    if (i % 3 == 1) {  // a share beside the certificates
      const int id = (int)(i % kN) + 1;
      r.signer = id;
      r.sig.resize(37);
      signers[id - 1]->signData(m.data(), (int)m.size(), r.sig.data(), 37);
      if (i % 15 == 7) r.sig[20] ^= 1;
      std::unique_ptr<IThresholdAccumulator> acc(kv.newAccumulator(true));
      acc->setExpectedDigest(reinterpret_cast<const unsigned char*>(m.data()), (int)m.size());
      r.want = acc->add(r.sig.data(), 37) == 1;
    } else {
      const int take = i % 10 == 8 ? kReq - 1 : (i % 4 == 3 ? kReq + 1 : kReq);  // too few / one more / k signers
      std::unique_ptr<IThresholdAccumulator> acc(kv.newAccumulator(false));
      for (int j = 0; j < take; j++) {
        char s[37];
        signers[(j + i % 3) % kN]->signData(m.data(), (int)m.size(), s, 37);  // three distinct sets, repeated
        acc->add(s, 37);
      }
      r.signer = 0;
      r.sig.resize((size_t)len);
      if (take >= kReq) {
        acc->getFullSignedData(r.sig.data(), len);
      } else {  // the accumulator does not combine fewer than k shares: the sum of two by hand, their bitmap
        BlsMultisigVerifier two(take, kN, vk);
        std::unique_ptr<IThresholdAccumulator> acc2(two.newAccumulator(false));
        for (int j = 0; j < take; j++) {
          char s[37];
          signers[(j + i % 3) % kN]->signData(m.data(), (int)m.size(), s, 37);
          acc2->add(s, 37);
        }
        acc2->getFullSignedData(r.sig.data(), len);
      }
      if (i % 12 == 5) r.msg = msgs[(i + 1) % msgs.size()];  // checked against another digest
      if (i % 14 == 6) r.sig[33 + 0] ^= (char)(1 << ((i / 14) % kN));  // a signer added to or dropped from the bitmap
      if (i % 16 == 9) r.sig[33 + 0] |= (char)(1 << kN);      // id 6 > numSigners
      if (i % 18 == 11) r.sig[33 + 255] |= (char)0x80;        // id 2048
      if (i % 20 == 12) r.sig.resize((size_t)len - 1);        // wrong lengths: false, no exception
      if (i % 22 == 14) r.sig.resize(33);
      if (i % 26 == 15) r.sig[5] ^= 4;                        // another x: a different point or none
      r.want = (int)r.sig.size() == len && kv.verify(r.msg.data(), (int)r.msg.size(), r.sig.data(), len);
      certs++;
    }
    valid += r.want;
    ref.push_back(r);
  }
  CHECK(valid > total / 3 && valid < total);
  CHECK(certs >= 2 * kMin);
  runSizes(kv, ref, "multisig k-of-n");

  // certificates alone, all under one bitmap and one digest
  {
    std::vector<Ref> same;
    for (const Ref& r : ref)
      if (r.signer == 0 && r.want) {
        for (size_t i = 0; i < kMin + 3; i++) same.push_back(r);
        break;
      }
    CHECK(!same.empty());
    same[1].sig[7] ^= 1;
    same[1].want = kv.verify(same[1].msg.data(), (int)same[1].msg.size(), same[1].sig.data(), len);
    runSizes(kv, same, "one set, one digest");
  }
}

int main(int argc, char** argv) {
  const bool noGpu = argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0;
  try {
    testNoGpu();
    if (!noGpu) testVerifyBatch();
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
