// Host-side test of BLS::Hip::BlsThresholdVerifier::verifyBatch: below the crossover (a loop of the
// lone calls), at it and above it (one cbft_bls_verify_batch) the verdicts are those of verify() and of
// the accumulator's share check, wrong-length entries included.
//
//   test_bls_verify_host            everything (needs the GPU)
//   test_bls_verify_host --no-gpu   the parts that never open the device: request validation, digest
//                                   deduplication, the crossover setting (the mode a sanitizer build
//                                   runs on a CPU-only machine)
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

static std::vector<std::string> makeMsgs(size_t count) {
  std::vector<std::string> msgs(count);
  uint32_t st = 4242;
  for (size_t i = 0; i < count; i++) {
    const size_t len = i == 1 ? 0 : i == 2 ? 1 : i == 3 ? 100 : 32;
    msgs[i].resize(len);
    for (auto& c : msgs[i]) c = (char)((st = st * 1664525u + 1013904223u) >> 24);
  }
  return msgs;
}

static void testNoGpu() {
  const char* e = std::getenv("CBFT_BLS_VERIFY_BATCH_MIN");
  const long long x = e ? std::atoll(e) : 0;
  CHECK(BlsThresholdVerifier::batchMin() == (x > 0 ? (size_t)x : (size_t)CBFT_BLS_VERIFY_BATCH_MIN_DEFAULT));

  std::vector<std::string> msgs = makeMsgs(6);
  std::vector<char> sig(40);
  for (size_t i = 0; i < sig.size(); i++) sig[i] = (char)(i + 1);
  std::vector<char> rec3(37, 7);  // a record of signer 3
  rec3[0] = rec3[1] = rec3[2] = 0;
  rec3[3] = 3;
  const std::string dup = msgs[4];  // equal bytes at another address
  std::vector<BlsVerifyRequest> r = {
      {msgs[0].data(), 32, sig.data(), 33, 0, true},      // 0: certificate
      {msgs[4].data(), 32, sig.data(), 33, 2, true},      // 1: 33-byte point of signer 2
      {dup.data(), 32, rec3.data(), 37, 3, true},         // 2: 37-byte record, same digest as 1
      {msgs[0].data(), 32, sig.data(), 32, 0, true},      // 3: short certificate
      {msgs[0].data(), 32, sig.data(), 37, 0, true},      // 4: a 37-byte entry is no certificate
      {msgs[0].data(), 32, sig.data(), 36, 1, true},      // 5: share of a wrong length
      {msgs[0].data(), 32, sig.data(), 40, 1, true},      // 6: share of a wrong length
      {msgs[0].data(), 32, sig.data(), 33, 6, true},      // 7: signer > numSigners
      {msgs[0].data(), 32, sig.data(), 33, -1, true},     // 8: negative signer
      {msgs[0].data(), 32, rec3.data(), 37, 4, true},     // 9: signer 3's record offered as signer 4's
      {nullptr, 32, sig.data(), 33, 0, true},             // 10
      {msgs[0].data(), -1, sig.data(), 33, 0, true},      // 11
      {msgs[0].data(), 32, nullptr, 33, 0, true},         // 12
      {msgs[1].data(), 0, sig.data(), 33, 5, true},       // 13: the empty message
      {msgs[3].data(), 100, sig.data(), 33, 0, true},     // 14: a long message
      {msgs[0].data(), 32, sig.data(), 33, 1, true},      // 15: digest of request 0 again
  };
  BlsVerifyPlan p;
  BlsThresholdVerifier::planBatch(r, 5, p);
  const std::vector<uint32_t> item = {0, 1, 2, 13, 14, 15}, key = {0, 2, 3, 5, 0, 1}, mof = {0, 1, 1, 2, 3, 0},
                              len = {32, 32, 0, 100};
  const std::vector<uint64_t> off = {0, 32, 64, 64};
  CHECK(p.item == item && p.keyIdx == key && p.msgOf == mof && p.msgLen == len && p.msgOff == off);
  CHECK(p.blob.size() == 164 && p.sig33.size() == 33 * item.size());
  CHECK(std::memcmp(p.blob.data(), msgs[0].data(), 32) == 0 && std::memcmp(p.blob.data() + 32, msgs[4].data(), 32) == 0);
  CHECK(std::memcmp(p.blob.data() + 64, msgs[3].data(), 100) == 0);
  CHECK(std::memcmp(&p.sig33[0], sig.data(), 33) == 0);
  CHECK(std::memcmp(&p.sig33[66], rec3.data() + 4, 33) == 0);  // the record's point, without its id
  for (const auto& q : r) CHECK(!q.ok);  // every verdict starts false; the refused ones stay so
  std::vector<BlsVerifyRequest> none;
  BlsThresholdVerifier::planBatch(none, 5, p);
  CHECK(p.item.empty() && p.blob.empty());
}

struct Ref {
  std::string msg;
  std::vector<char> sig;
  ShareID signer;
  bool want;
};

// what the accumulator's share check says about one 37-byte (or wrong-length) record
static bool accumulatorAccepts(const BlsThresholdVerifier& v, const std::string& msg, const char* rec, int len) {
  std::unique_ptr<IThresholdAccumulator> acc(v.newAccumulator(true));
  acc->setExpectedDigest(reinterpret_cast<const unsigned char*>(msg.data()), (int)msg.size());
  return acc->add(rec, len) == 1;
}

static void runSizes(const BlsThresholdVerifier& v, const std::vector<Ref>& ref, const char* what) {
  const size_t kMin = BlsThresholdVerifier::batchMin(), total = ref.size();
  for (size_t n : {(size_t)0, (size_t)1, kMin - 1, kMin, kMin + 1, total}) {
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
  const char* masterDec = "7934650183025465912345678901234567890123456789012345678901234567890123";
  std::vector<std::unique_ptr<BlsThresholdSigner>> signers;
  std::vector<std::string> vk;
  for (int i = 0; i < kN; i++) {
    signers.emplace_back(new BlsThresholdSigner(i + 1, skDec[i]));
    vk.push_back(signers.back()->getShareVerificationKey().toString());
  }
  BlsThresholdSigner master(1, masterDec);  // its "share" is sk * H: the combined signature under sk * g2
  BlsThresholdVerifier v(master.getShareVerificationKey().toString(), kReq, kN, vk);
  const size_t kMin = BlsThresholdVerifier::batchMin(), total = kMin + 36;
  std::vector<std::string> msgs = makeMsgs(9);  // few digests, many entries: the batch deduplicates
  msgs.erase(msgs.begin() + 1);                 // (an accumulator takes no empty digest)
  std::vector<Ref> ref;
  size_t valid = 0;
  for (size_t i = 0; i < total; i++) {
    const std::string& m = msgs[i % msgs.size()];
    const std::string& other = msgs[(i + 1) % msgs.size()];
    Ref r;
    r.msg = m;
    std::vector<char> s(37);
    if (i % 3 == 0) {  // certificate
      r.signer = 0;
      master.signData((i % 9 == 6 ? other : m).data(), (int)(i % 9 == 6 ? other : m).size(), s.data(), 37);
      r.sig.assign(s.begin() + 4, s.end());
      if (i % 12 == 9) r.sig.resize(32);       // wrong length
      if (i % 24 == 3) r.sig.assign(s.begin(), s.end());  // 37 bytes: no certificate
      r.want = v.verify(r.msg.data(), (int)r.msg.size(), r.sig.data(), (int)r.sig.size());
    } else {  // share
      const int id = (int)(i % kN) + 1;
      r.signer = id;
      signers[id - 1]->signData((i % 7 == 4 ? other : m).data(), (int)(i % 7 == 4 ? other : m).size(), s.data(), 37);
      if (i % 11 == 5) s[20] ^= 1;  // another x: a different point or none
      std::vector<char> rec = s;
      if (i % 13 == 7) rec.resize(36);
      if (i % 17 == 8) rec.resize(40, 0);
      r.want = accumulatorAccepts(v, r.msg, rec.data(), (int)rec.size());
      if (rec.size() == 37 && i % 2) rec.erase(rec.begin(), rec.begin() + 4);  // the 33-byte point alone
      r.sig = rec;
    }
    valid += r.want;
    ref.push_back(r);
  }
  CHECK(valid > total / 3 && valid < total);
  runSizes(v, ref, "threshold");

  // out-of-range signers and a record under another signer's id: false, no exception
  {
    std::vector<BlsVerifyRequest> reqs;
    for (size_t i = 0; i < kMin + 2; i++) {
      const Ref& r = ref[1];  // a share
      reqs.push_back({r.msg.data(), (int)r.msg.size(), r.sig.data(), (int)r.sig.size(), r.signer, false});
    }
    reqs[0].signer = kN + 1;
    reqs[1].signer = 2048;
    v.verifyBatch(reqs);
    CHECK(!reqs[0].ok && !reqs[1].ok && reqs[2].ok == ref[1].want);
  }

  // n-of-n multisig: PK = sum of the vk_i; 33-byte signatures through the batch
  {
    BlsMultisigVerifier mv(kN, kN, vk);
    std::vector<Ref> mref;
    for (size_t i = 0; i < kMin + 6; i++) {
      const std::string& m = msgs[i % 3];
      std::unique_ptr<IThresholdAccumulator> acc(mv.newAccumulator(false));
      for (int j = 0; j < kN; j++) {
        char s[37];
        signers[j]->signData(m.data(), (int)m.size(), s, 37);
        acc->add(s, 37);
      }
      Ref r;
      r.msg = i % 4 == 2 ? msgs[5] : m;  // every 4th is checked against another digest
      r.sig.resize(33);
      acc->getFullSignedData(r.sig.data(), 33);
      r.signer = 0;
      r.want = mv.verify(r.msg.data(), (int)r.msg.size(), r.sig.data(), 33);
      CHECK(r.want == (i % 4 != 2));
      mref.push_back(r);
    }
    runSizes(mv, mref, "multisig n-of-n");
  }
  // k-of-n multisig: the signature carries its signer bitmap and goes through verify()
  {
    BlsMultisigVerifier kv(kReq, kN, vk);
    const int len = kv.requiredLengthForSignedData();
    std::vector<Ref> kref;
    for (size_t i = 0; i < kMin + 3; i++) {
      const std::string& m = msgs[i % 3];
      Ref r;
      r.msg = m;
      if (i % 2) {  // a share beside the certificates
        r.signer = 2;
        r.sig.resize(37);
        signers[1]->signData(m.data(), (int)m.size(), r.sig.data(), 37);
        r.want = true;
      } else {
        std::unique_ptr<IThresholdAccumulator> acc(kv.newAccumulator(false));
        for (int j = 0; j < kReq; j++) {
          char s[37];
          signers[(j + i) % kN]->signData(m.data(), (int)m.size(), s, 37);
          acc->add(s, 37);
        }
        r.sig.resize((size_t)len);
        acc->getFullSignedData(r.sig.data(), len);
        if (i % 4 == 2) r.msg = msgs[6];
        r.signer = 0;
        r.want = kv.verify(r.msg.data(), (int)r.msg.size(), r.sig.data(), len);
        CHECK(r.want == (i % 4 != 2));
      }
      kref.push_back(r);
    }
    runSizes(kv, kref, "multisig k-of-n");
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
