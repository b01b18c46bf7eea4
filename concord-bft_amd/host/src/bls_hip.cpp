// BLS::Hip threshold verifier / accumulator / signer over libcbft_hipcrypto (see bls_hip.hpp).
#include "threshsign/bls_hip.hpp"

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <unordered_map>

#include <openssl/bn.h>
#include <openssl/crypto.h>
#include <openssl/rand.h>

#include "cbft_hipcrypto.h"

namespace BLS {
namespace Hip {

// ------------------------------------------------------------------------------ engine
class BlsEngine {
 public:
  static std::shared_ptr<BlsEngine> get() {
    static std::mutex m;
    static std::weak_ptr<BlsEngine> inst;
    std::lock_guard<std::mutex> g(m);
    auto sp = inst.lock();
    if (!sp) {
      sp = std::shared_ptr<BlsEngine>(new BlsEngine());
      inst = sp;
    }
    return sp;
  }
  ~BlsEngine() {
    if (ctx_) cbft_close(ctx_);
  }
  cbft_ctx* ctx() const { return ctx_; }

 private:
  BlsEngine() {
    const char* d = std::getenv("CBFT_DEVICE");
    int rc = cbft_open(&ctx_, d ? std::atoi(d) : 0, 0);
    if (rc) throw std::runtime_error(std::string("cbft_open: ") + cbft_strerror(rc) + " " + cbft_last_error());
  }
  cbft_ctx* ctx_ = nullptr;
};

static void check(int rc, const char* what) {
  if (rc) throw std::runtime_error(std::string(what) + ": " + cbft_strerror(rc) + " " + cbft_last_error());
}

static int hexval(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  if (c >= 'A' && c <= 'F') return c - 'A' + 10;
  return -1;
}

// ------------------------------------------------------------------------------ keys
BlsPublicKey::BlsPublicKey(const std::string& hex) : hex_(hex) {
  if (hex.size() != 130) throw std::invalid_argument("BLS G2 key: expected 130 hex characters");
  for (size_t i = 0; i < 65; i++) {
    int a = hexval(hex[2 * i]), b = hexval(hex[2 * i + 1]);
    if (a < 0 || b < 0) throw std::invalid_argument("BLS G2 key: not hex");
    raw_[i] = (uint8_t)(a * 16 + b);
  }
}

static std::string toHex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s(2 * n, '0');
  for (size_t i = 0; i < n; i++) {
    s[2 * i] = d[p[i] >> 4];
    s[2 * i + 1] = d[p[i] & 15];
  }
  return s;
}

BlsSecretKey::BlsSecretKey(const std::string& decimal) : dec_(decimal) {
  if (decimal.empty()) throw std::invalid_argument("BLS secret key: empty");
  for (char ch : decimal) {  // be_ = be_ * 10 + digit, big-endian bytes
    if (ch < '0' || ch > '9') throw std::invalid_argument("BLS secret key: not a decimal number");
    unsigned carry = (unsigned)(ch - '0');
    for (int i = 31; i >= 0; i--) {
      unsigned v = be_[i] * 10u + carry;
      be_[i] = (uint8_t)v;
      carry = v >> 8;
    }
    if (carry) throw std::invalid_argument("BLS secret key: exceeds 256 bits");
  }
}

BlsSecretKey::BlsSecretKey(const std::array<uint8_t, 32>& bigEndian) : be_(bigEndian) {
  // decimal digits by repeated division by 10 (most significant byte first)
  std::array<uint8_t, 32> t = bigEndian;
  std::string rev;
  for (;;) {
    unsigned rem = 0, any = 0;
    for (size_t i = 0; i < 32; i++) {
      const unsigned v = rem * 256u + t[i];
      t[i] = (uint8_t)(v / 10u);
      rem = v % 10u;
      any |= t[i];
    }
    rev.push_back((char)('0' + rem));
    if (!any) break;
  }
  dec_.assign(rev.rbegin(), rev.rend());
  OPENSSL_cleanse(&rev[0], rev.size());
  OPENSSL_cleanse(t.data(), t.size());
}

BlsSecretKey::~BlsSecretKey() {
  if (!dec_.empty()) OPENSSL_cleanse(&dec_[0], dec_.size());
  OPENSSL_cleanse(be_.data(), be_.size());
}

// ------------------------------------------------------------------------------ verifiers
BlsThresholdVerifier::BlsThresholdVerifier(const std::string& pkHex, NumSharesType reqSigners,
                                           NumSharesType numSigners, const std::vector<std::string>& vkHex)
    : req_(reqSigners), num_(numSigners) {
  if (numSigners < 1 || numSigners > MAX_NUM_OF_SHARES || reqSigners < 1 || reqSigners > numSigners)
    throw std::invalid_argument("BLS verifier: need 1 <= reqSigners <= numSigners <= 2048");
  if (vkHex.size() != (size_t)numSigners) throw std::invalid_argument("BLS verifier: need numSigners keys");
  if (!pkHex.empty()) pk_ = BlsPublicKey(pkHex);
  vks_.reserve(vkHex.size());
  std::vector<uint8_t> vk65(65 * vkHex.size());
  for (size_t i = 0; i < vkHex.size(); i++) {
    vks_.emplace_back(vkHex[i]);
    std::memcpy(&vk65[65 * i], vks_.back().bytes().data(), 65);
  }
  engine_ = BlsEngine::get();
  check(cbft_bls_load_keys(engine_->ctx(), pk_.bytes().data(), vk65.data(), (uint32_t)numSigners, &keyset_),
        "cbft_bls_load_keys");
}

BlsThresholdVerifier::~BlsThresholdVerifier() {
  if (engine_) (void)cbft_bls_unload_keys(engine_->ctx(), keyset_);
}

const IShareVerificationKey& BlsThresholdVerifier::getShareVerificationKey(ShareID signer) const {
  if (signer < 1 || signer > num_) throw std::out_of_range("BLS verifier: signer id out of range");
  return vks_[(size_t)signer - 1];
}

IThresholdAccumulator* BlsThresholdVerifier::newAccumulator(bool withShareVerification) const {
  // k = n - 1 takes the reference's "almost multisig" accumulator, which never verifies shares
  // (BlsThresholdVerifier.cpp:61-67); its precomputed coefficients equal the Lagrange ones.
  if (req_ == num_ - 1) return new BlsThresholdAccumulator(*this, req_, false);
  return new BlsThresholdAccumulator(*this, req_, withShareVerification);
}

bool BlsThresholdVerifier::verify(const char* msg, int msgLen, const char* sig, int sigLen) const {
  if (!msg || msgLen < 0 || !sig || sigLen != 33) return false;
  int ok = 0;
  check(cbft_bls_verify(engine_->ctx(), keyset_, reinterpret_cast<const uint8_t*>(msg), (uint32_t)msgLen,
                        reinterpret_cast<const uint8_t*>(sig), &ok),
        "cbft_bls_verify");
  return ok != 0;
}

static void putRecord(std::vector<uint8_t>& out, ShareID id, const uint8_t* s33);

size_t BlsThresholdVerifier::batchMin() {
  static const size_t v = [] {
    const char* e = std::getenv("CBFT_BLS_VERIFY_BATCH_MIN");
    const long long x = e ? std::atoll(e) : 0;
    return x > 0 ? (size_t)x : (size_t)CBFT_BLS_VERIFY_BATCH_MIN_DEFAULT;
  }();
  return v;
}

void BlsThresholdVerifier::planBatch(std::vector<BlsVerifyRequest>& requests, NumSharesType numSigners,
                                     BlsVerifyPlan& plan) {
  plan = BlsVerifyPlan();
  std::unordered_map<std::string, uint32_t> seen;  // message bytes -> its index in the plan
  for (size_t i = 0; i < requests.size(); i++) {
    BlsVerifyRequest& r = requests[i];
    r.ok = false;
    if (!r.msg || r.msgLen < 0 || !r.sig) continue;
    const uint8_t* s = reinterpret_cast<const uint8_t*>(r.sig);
    if (r.signer == 0) {
      if (r.sigLen != 33) continue;  // verify(): false
    } else {
      if (r.signer < 1 || r.signer > numSigners) continue;
      if (r.sigLen == 37) {
        const uint32_t id = ((uint32_t)s[0] << 24) | ((uint32_t)s[1] << 16) | ((uint32_t)s[2] << 8) | s[3];
        if (id != (uint32_t)r.signer) continue;  // another signer's record
        s += 4;
      } else if (r.sigLen != 33) {
        continue;  // add(): a point that never decodes
      }
    }
    std::string key(r.msg, (size_t)r.msgLen);
    auto it = seen.find(key);
    if (it == seen.end()) {
      it = seen.emplace(std::move(key), (uint32_t)plan.msgLen.size()).first;
      plan.msgOff.push_back(plan.blob.size());
      plan.msgLen.push_back((uint32_t)r.msgLen);
      plan.blob.insert(plan.blob.end(), r.msg, r.msg + r.msgLen);
    }
    plan.item.push_back((uint32_t)i);
    plan.keyIdx.push_back((uint32_t)r.signer);
    plan.msgOf.push_back(it->second);
    plan.sig33.insert(plan.sig33.end(), s, s + 33);
  }
}

void BlsThresholdVerifier::verifyBatch(std::vector<BlsVerifyRequest>& requests) const {
  BlsVerifyPlan p;
  planBatch(requests, num_, p);
  const size_t n = p.item.size();
  if (n == 0) return;
  if (requests.size() < batchMin()) {
    for (size_t j = 0; j < n; j++) {
      BlsVerifyRequest& r = requests[p.item[j]];
      const uint8_t* s33 = &p.sig33[33 * j];
      if (r.signer == 0) {
        r.ok = verify(r.msg, r.msgLen, reinterpret_cast<const char*>(s33), 33);
        continue;
      }
      std::vector<uint8_t> rec;
      putRecord(rec, r.signer, s33);
      uint8_t bit = 0;
      check(cbft_bls_verify_shares(engine_->ctx(), keyset_, reinterpret_cast<const uint8_t*>(r.msg), (uint32_t)r.msgLen,
                                   rec.data(), 1, &bit),
            "cbft_bls_verify_shares");
      r.ok = (bit & 1) != 0;
    }
    return;
  }
  if (p.blob.empty()) p.blob.push_back(0);
  std::vector<uint8_t> bits((n + 7) / 8);
  check(cbft_bls_verify_batch(engine_->ctx(), keyset_, p.keyIdx.data(), p.sig33.data(), p.blob.data(), p.msgOff.data(),
                              p.msgLen.data(), p.msgLen.size(), p.msgOf.data(), n, bits.data()),
        "cbft_bls_verify_batch");
  for (size_t j = 0; j < n; j++) requests[p.item[j]].ok = ((bits[j >> 3] >> (j & 7)) & 1) != 0;
}

static std::vector<uint8_t> allSigners(NumSharesType n) {
  VectorOfShares v;
  for (ShareID i = 1; i <= n; i++) v.add(i);
  std::vector<uint8_t> b((size_t)VectorOfShares::getByteCount());
  v.toBytes(b.data(), (int)b.size());
  return b;
}

BlsMultisigVerifier::BlsMultisigVerifier(NumSharesType reqSigners, NumSharesType numSigners,
                                         const std::vector<std::string>& vkHex)
    : BlsThresholdVerifier("", reqSigners, numSigners, vkHex) {
  if (req_ == num_) {  // PK = sum of all vk_i; reload the key set with it in slot 0
    uint8_t pk65[65];
    std::vector<uint8_t> all = allSigners(num_);
    check(cbft_bls_sum_keys(engine_->ctx(), keyset_, all.data(), pk65), "cbft_bls_sum_keys");
    pk_ = BlsPublicKey(toHex(pk65, 65));
    std::vector<uint8_t> vk65(65 * vks_.size());
    for (size_t i = 0; i < vks_.size(); i++) std::memcpy(&vk65[65 * i], vks_[i].bytes().data(), 65);
    uint32_t id = 0;
    check(cbft_bls_load_keys(engine_->ctx(), pk65, vk65.data(), (uint32_t)num_, &id), "cbft_bls_load_keys");
    (void)cbft_bls_unload_keys(engine_->ctx(), keyset_);
    keyset_ = id;
  }
}

IThresholdAccumulator* BlsMultisigVerifier::newAccumulator(bool withShareVerification) const {
  return new BlsMultisigAccumulator(*this, req_, withShareVerification);
}

int BlsMultisigVerifier::requiredLengthForSignedData() const {
  return 33 + (req_ != num_ ? VectorOfShares::getByteCount() : 0);
}

bool BlsMultisigVerifier::verify(const char* msg, int msgLen, const char* sig, int sigLen) const {
  if (req_ == num_) return BlsThresholdVerifier::verify(msg, msgLen, sig, 33);
  if (sigLen != requiredLengthForSignedData()) throw std::runtime_error("Signature does not have the right size");
  if (!msg || msgLen < 0 || !sig) return false;
  VectorOfShares signers;
  signers.fromBytes(reinterpret_cast<const unsigned char*>(sig) + 33, VectorOfShares::getByteCount());
  if (signers.count() < req_) return false;
  for (ShareID id = signers.first(); !signers.isEnd(id); id = signers.next(id))
    if (id > num_) return false;  // no such signer (the reference would index past its key vector)
  int ok = 0;
  check(cbft_bls_verify_multisig(engine_->ctx(), keyset_, reinterpret_cast<const uint8_t*>(msg), (uint32_t)msgLen,
                                 reinterpret_cast<const uint8_t*>(sig),
                                 reinterpret_cast<const uint8_t*>(sig) + 33, &ok),
        "cbft_bls_verify_multisig");
  return ok != 0;
}

size_t BlsMultisigVerifier::multisigBatchMin() {
  static const size_t v = [] {
    const char* e = std::getenv("CBFT_BLS_MULTISIG_BATCH_MIN");
    const long long x = e ? std::atoll(e) : 0;
    return x > 0 ? (size_t)x : (size_t)CBFT_BLS_MULTISIG_BATCH_MIN_DEFAULT;
  }();
  return v;
}

void BlsMultisigVerifier::planMultisigBatch(std::vector<BlsVerifyRequest>& requests, NumSharesType reqSigners,
                                            NumSharesType numSigners, BlsMultisigPlan& plan) {
  plan = BlsMultisigPlan();
  const size_t setLen = (size_t)VectorOfShares::getByteCount();
  std::unordered_map<std::string, uint32_t> seenMsg, seenSet;  // bytes -> index in the plan
  for (size_t i = 0; i < requests.size(); i++) {
    BlsVerifyRequest& r = requests[i];
    if (r.signer != 0) continue;
    r.ok = false;
    if (r.sigLen != 33 + (int)setLen || !r.msg || r.msgLen < 0 || !r.sig) continue;
    const uint8_t* s = reinterpret_cast<const uint8_t*>(r.sig);
    const uint8_t* bm = s + 33;
    // verify()'s rules: at least reqSigners signers, none above numSigners
    size_t count = 0;
    bool above = false;
    for (size_t q = 0; q < setLen; q++)
      for (int t = 0; t < 8; t++)
        if ((bm[q] >> t) & 1) {
          count++;
          above = above || 8 * q + t + 1 > (size_t)numSigners;
        }
    if (count < (size_t)reqSigners || above) continue;
    std::string mkey(r.msg, (size_t)r.msgLen);
    auto mi = seenMsg.find(mkey);
    if (mi == seenMsg.end()) {
      mi = seenMsg.emplace(std::move(mkey), (uint32_t)plan.msgLen.size()).first;
      plan.msgOff.push_back(plan.blob.size());
      plan.msgLen.push_back((uint32_t)r.msgLen);
      plan.blob.insert(plan.blob.end(), r.msg, r.msg + r.msgLen);
    }
    std::string skey(reinterpret_cast<const char*>(bm), setLen);
    auto si = seenSet.find(skey);
    if (si == seenSet.end()) {
      si = seenSet.emplace(std::move(skey), (uint32_t)(plan.sets.size() / setLen)).first;
      plan.sets.insert(plan.sets.end(), bm, bm + setLen);
    }
    plan.item.push_back((uint32_t)i);
    plan.setOf.push_back(si->second);
    plan.msgOf.push_back(mi->second);
    plan.sig33.insert(plan.sig33.end(), s, s + 33);
  }
}

void BlsMultisigVerifier::verifyBatch(std::vector<BlsVerifyRequest>& requests) const {
  if (req_ == num_) return BlsThresholdVerifier::verifyBatch(requests);
  // the shares as one batch; the k-of-n signatures, each under its own key sum, as another
  std::vector<BlsVerifyRequest> shares;
  std::vector<size_t> at;
  for (size_t i = 0; i < requests.size(); i++)
    if (requests[i].signer != 0) {
      shares.push_back(requests[i]);
      at.push_back(i);
    }
  BlsMultisigPlan p;
  planMultisigBatch(requests, req_, num_, p);
  const size_t n = p.item.size();
  if (n && n < multisigBatchMin()) {
    for (size_t j = 0; j < n; j++) {
      BlsVerifyRequest& r = requests[p.item[j]];
      r.ok = verify(r.msg, r.msgLen, r.sig, r.sigLen);
    }
  } else if (n) {
    if (p.blob.empty()) p.blob.push_back(0);
    std::vector<uint8_t> bits((n + 7) / 8);
    check(cbft_bls_verify_multisig_batch(engine_->ctx(), keyset_, p.sets.data(), p.sets.size() / 256, p.setOf.data(),
                                         p.sig33.data(), p.blob.data(), p.msgOff.data(), p.msgLen.data(),
                                         p.msgLen.size(), p.msgOf.data(), n, bits.data()),
          "cbft_bls_verify_multisig_batch");
    for (size_t j = 0; j < n; j++) requests[p.item[j]].ok = ((bits[j >> 3] >> (j & 7)) & 1) != 0;
  }
  BlsThresholdVerifier::verifyBatch(shares);
  for (size_t j = 0; j < at.size(); j++) requests[at[j]].ok = shares[j].ok;
}

// ------------------------------------------------------------------------------ accumulators
BlsAccumulatorBase::BlsAccumulatorBase(const BlsThresholdVerifier& v, NumSharesType reqSigners,
                                       bool withShareVerification)
    : v_(v),
      req_(reqSigners),
      num_(v.getNumTotalShares()),
      verify_(withShareVerification),
      pending_((size_t)num_ + 1),
      valid_((size_t)num_ + 1) {}

int BlsAccumulatorBase::getNumValidShares() const {
  return (!verify_ || hasExpectedDigest()) ? validBits_.count() : 0;
}

// BlsSigshareParser (BlsAccumulatorBase.cpp:33-43): 4-byte big-endian id, then the G1 point.
int BlsAccumulatorBase::add(const char* sigShare, int len) {
  if (!sigShare || len < 4) throw std::invalid_argument("BLS share: shorter than its id");
  const uint8_t* b = reinterpret_cast<const uint8_t*>(sigShare);
  const ShareID id = (ShareID)(((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3]);
  uint8_t s[33];
  if (len - 4 == 33) {
    std::memcpy(s, b + 4, 33);
  } else {
    std::memset(s, 0xff, 33);  // wrong length: a point that never decodes (RELIC would error)
  }
  return addNumById(id, s);
}

static void putRecord(std::vector<uint8_t>& out, ShareID id, const uint8_t* s33) {
  out.push_back((uint8_t)(id >> 24));
  out.push_back((uint8_t)(id >> 16));
  out.push_back((uint8_t)(id >> 8));
  out.push_back((uint8_t)id);
  out.insert(out.end(), s33, s33 + 33);
}

// ThresholdAccumulatorBase::addNumById (ThresholdAccumulatorBase.cpp:87-147)
int BlsAccumulatorBase::addNumById(ShareID signer, const uint8_t* share33) {
  if (signer < 1 || signer > num_) {  // reference: debug assert; here the share is refused
    invalid_.insert(signer);
    return (verify_ && !hasExpectedDigest()) ? pendingBits_.count() : validBits_.count();
  }
  const size_t idx = (size_t)signer;
  if (verify_ && !hasExpectedDigest()) {
    if (!pendingBits_.contains(signer)) {
      std::memcpy(pending_[idx].data(), share33, 33);
      pendingBits_.add(signer);
    }
    return pendingBits_.count();
  }
  if (validBits_.count() == req_) return validBits_.count();
  if (!validBits_.contains(signer)) {
    bool ok = true;
    if (verify_) {
      std::vector<uint8_t> rec;
      putRecord(rec, signer, share33);
      uint8_t bit = 0;
      check(cbft_bls_verify_shares(v_.engine()->ctx(), v_.keysetId(), digest_.data(), (uint32_t)digest_.size(),
                                   rec.data(), 1, &bit),
            "cbft_bls_verify_shares");
      ok = (bit & 1) != 0;
    }
    if (ok) {
      std::memcpy(valid_[idx].data(), share33, 33);
      validBits_.add(signer);
    }
  }
  return validBits_.count();
}

// ThresholdAccumulatorBase::setExpectedDigest (ThresholdAccumulatorBase.cpp:19-57)
void BlsAccumulatorBase::setExpectedDigest(const unsigned char* msg, int len) {
  if (!msg || len <= 0) throw std::invalid_argument("setExpectedDigest: empty digest");
  if (!hasExpectedDigest()) {
    digest_.assign(msg, msg + len);
    if (verify_) verifyPendingShares();
    return;
  }
  if ((int)digest_.size() != len) throw std::runtime_error("Cannot reset expected digest with different length");
  if (std::memcmp(digest_.data(), msg, (size_t)len) != 0)
    throw std::runtime_error("Cannot reset expected digest to a different one");
}

// All pending shares in one launch, then the reference's walk (ThresholdAccumulatorBase.cpp:59-85):
// id order, stop once reqSigners are valid, failed ones before that point reported invalid.
void BlsAccumulatorBase::verifyPendingShares() {
  std::vector<ShareID> ids;
  std::vector<uint8_t> recs;
  for (ShareID id = pendingBits_.first(); !pendingBits_.isEnd(id); id = pendingBits_.next(id)) {
    ids.push_back(id);
    putRecord(recs, id, pending_[(size_t)id].data());
  }
  if (!ids.empty()) {
    std::vector<uint8_t> bits((ids.size() + 7) / 8);
    check(cbft_bls_verify_shares(v_.engine()->ctx(), v_.keysetId(), digest_.data(), (uint32_t)digest_.size(),
                                 recs.data(), (uint32_t)ids.size(), bits.data()),
          "cbft_bls_verify_shares");
    for (size_t j = 0; j < ids.size(); j++) {
      if (validBits_.count() == req_) break;
      const ShareID id = ids[j];
      if ((bits[j >> 3] >> (j & 7)) & 1) {
        valid_[(size_t)id] = pending_[(size_t)id];
        validBits_.add(id);
      } else {
        invalid_.insert(id);
      }
    }
  }
  pending_.clear();
}

std::vector<uint8_t> BlsAccumulatorBase::validRecords() const {
  std::vector<uint8_t> recs;
  for (ShareID id = validBits_.first(); !validBits_.isEnd(id); id = validBits_.next(id))
    putRecord(recs, id, valid_[(size_t)id].data());
  return recs;
}

static void combineInto(const BlsThresholdVerifier& v, const std::vector<uint8_t>& recs, int multisig,
                        uint8_t* out33) {
  const uint32_t k = (uint32_t)(recs.size() / 37);
  if (k == 0) {  // identity (G1T::Identity(), BlsThresholdAccumulator.cpp:34)
    std::memset(out33, 0, 33);
    return;
  }
  check(cbft_bls_combine(v.engine()->ctx(), recs.data(), k, multisig, out33), "cbft_bls_combine");
}

void BlsThresholdAccumulator::getFullSignedData(char* out, int len) {
  if (!out || len < 33) throw std::runtime_error("Not enough capacity to store threshold signature");
  combineInto(v_, validRecords(), 0, reinterpret_cast<uint8_t*>(out));
}

void BlsMultisigAccumulator::getFullSignedData(char* out, int len) {
  const int vec = (req_ != num_) ? VectorOfShares::getByteCount() : 0;
  if (!out || len < 33 + vec) throw std::runtime_error("Not enough capacity to store multisignature");
  combineInto(v_, validRecords(), 1, reinterpret_cast<uint8_t*>(out));
  if (vec) validBits_.toBytes(reinterpret_cast<unsigned char*>(out) + 33, vec);
}

// ------------------------------------------------------------------------------ batched combination
void BlsAccumulatorBase::combineInput(BlsCombineInput& in) const {
  in.usable = true;
  in.multisig = multisig();
  in.records = validRecords();
  in.signers.clear();
  if (in.multisig && req_ != num_) {
    in.signers.resize((size_t)VectorOfShares::getByteCount());
    validBits_.toBytes(in.signers.data(), (int)in.signers.size());
  }
}

size_t combineBatchMin() {
  static const size_t v = [] {
    const char* e = std::getenv("CBFT_BLS_COMBINE_BATCH_MIN");
    const long long x = e ? std::atoll(e) : 0;
    return x > 0 ? (size_t)x : (size_t)CBFT_BLS_COMBINE_BATCH_MIN_DEFAULT;
  }();
  return v;
}

void planCombine(const std::vector<BlsCombineInput>& in, std::vector<BlsCombineRequest>& requests, BlsCombinePlan& plan) {
  if (in.size() != requests.size()) throw std::invalid_argument("planCombine: one input per request");
  plan = BlsCombinePlan();
  plan.certOff.push_back(0);
  bool kindKnown = false;
  for (size_t i = 0; i < requests.size(); i++) {
    BlsCombineRequest& r = requests[i];
    const BlsCombineInput& a = in[i];
    r.ok = false;
    if (!a.usable) continue;
    if (kindKnown && a.multisig != plan.multisig) throw std::invalid_argument("combineBatch: accumulators of two kinds");
    plan.multisig = a.multisig;
    kindKnown = true;
    if (a.records.size() % 37 != 0) throw std::invalid_argument("planCombine: records are 37 bytes each");
    if (!r.out || r.outLen < 0 || (size_t)r.outLen < 33 + a.signers.size()) continue;  // getFullSignedData throws
    if (a.records.empty()) {  // the identity (G1T::Identity(), BlsThresholdAccumulator.cpp:34)
      std::memset(r.out, 0, 33);
      if (!a.signers.empty()) std::memcpy(r.out + 33, a.signers.data(), a.signers.size());
      r.ok = true;
      continue;
    }
    plan.item.push_back((uint32_t)i);
    plan.shares37.insert(plan.shares37.end(), a.records.begin(), a.records.end());
    plan.certOff.push_back(plan.shares37.size() / 37);
  }
}

void combineBatch(std::vector<BlsCombineRequest>& requests) {
  const BlsThresholdVerifier* v = nullptr;
  std::vector<BlsCombineInput> in(requests.size());
  for (size_t i = 0; i < requests.size(); i++) {
    const auto* a = dynamic_cast<const BlsAccumulatorBase*>(requests[i].acc);
    if (!a) continue;
    if (v && v != &a->verifier()) throw std::invalid_argument("combineBatch: accumulators of different verifiers");
    v = &a->verifier();
    if (requests.size() >= combineBatchMin()) a->combineInput(in[i]);
  }
  if (requests.size() < combineBatchMin()) {
    for (BlsCombineRequest& r : requests) {
      r.ok = false;
      if (!dynamic_cast<const BlsAccumulatorBase*>(r.acc)) continue;
      try {
        r.acc->getFullSignedData(r.out, r.outLen);
        r.ok = true;
      } catch (const std::runtime_error&) {
      }
    }
    return;
  }
  BlsCombinePlan p;
  planCombine(in, requests, p);
  const size_t m = p.item.size();
  if (m == 0) return;
  std::vector<uint8_t> sig(33 * m), status(m);
  check(cbft_bls_combine_batch(v->engine()->ctx(), p.shares37.data(), p.certOff.data(), m, nullptr, p.multisig ? 1 : 0,
                               sig.data(), status.data()),
        "cbft_bls_combine_batch");
  for (size_t j = 0; j < m; j++) {
    if (!status[j]) continue;
    BlsCombineRequest& r = requests[p.item[j]];
    std::memcpy(r.out, &sig[33 * j], 33);
    const std::vector<uint8_t>& tail = in[p.item[j]].signers;
    if (!tail.empty()) std::memcpy(r.out + 33, tail.data(), tail.size());
    r.ok = true;
  }
}

// ------------------------------------------------------------------------------ signer
BlsThresholdSigner::BlsThresholdSigner(ShareID id, const std::string& secretKeyDecimal, const std::string& vkHex)
    : id_(id), sk_(secretKeyDecimal), vk_(vkHex.empty() ? BlsPublicKey() : BlsPublicKey(vkHex)) {
  if (id < 1 || id > MAX_NUM_OF_SHARES) throw std::invalid_argument("BLS signer: id out of range");
  engine_ = BlsEngine::get();
  if (vkHex.empty()) {  // the reference derives it: publicKey_(secretKey) = sk * g2 (BlsThresholdSigner.cpp:25)
    uint8_t vk65[65];
    check(cbft_bls_public_key(engine_->ctx(), sk_.bytes().data(), vk65), "cbft_bls_public_key");
    vk_ = BlsPublicKey(toHex(vk65, 65));
  }
}

void BlsThresholdSigner::signData(const char* hash, int hashLen, char* outSig, int outSigLen) {
  if (!outSig || outSigLen < 37) throw std::runtime_error("BLS signer: output buffer shorter than 37 bytes");
  if (!hash || hashLen < 0) throw std::invalid_argument("BLS signer: no message");
  check(cbft_bls_sign(engine_->ctx(), sk_.bytes().data(), (uint32_t)id_, reinterpret_cast<const uint8_t*>(hash),
                      (uint32_t)hashLen, reinterpret_cast<uint8_t*>(outSig)),
        "cbft_bls_sign");
}

BlsThresholdSigner::~BlsThresholdSigner() {
  if (signer_table_) (void)cbft_bls_unload_signers(engine_->ctx(), signer_table_);
}

size_t BlsThresholdSigner::batchMin() {
  static const size_t v = [] {
    const char* e = std::getenv("CBFT_BLS_SIGN_BATCH_MIN");
    const long long x = e ? std::atoll(e) : 0;
    return x > 0 ? (size_t)x : (size_t)CBFT_BLS_SIGN_BATCH_MIN_DEFAULT;
  }();
  return v;
}

void BlsThresholdSigner::signBatch(const std::vector<BlsSignRequest>& requests) {
  for (const auto& r : requests) {
    if (!r.out || r.outLen < 37) throw std::runtime_error("BLS signer: output buffer shorter than 37 bytes");
    if (!r.hash || r.hashLen < 0) throw std::invalid_argument("BLS signer: no message");
  }
  const size_t n = requests.size();
  if (n < batchMin()) {
    for (const auto& r : requests) signData(r.hash, r.hashLen, r.out, r.outLen);
    return;
  }
  {
    std::lock_guard<std::mutex> g(table_mu_);
    if (!signer_table_) {
      const uint32_t id = (uint32_t)id_;
      check(cbft_bls_load_signers(engine_->ctx(), sk_.bytes().data(), &id, 1, &signer_table_), "cbft_bls_load_signers");
    }
  }
  std::vector<uint64_t> off(n);
  std::vector<uint32_t> len(n);
  size_t total = 0;
  for (size_t i = 0; i < n; i++) {
    off[i] = total;
    len[i] = (uint32_t)requests[i].hashLen;
    total += len[i];
  }
  std::vector<uint8_t> blob(total ? total : 1), out(37 * n);
  for (size_t i = 0; i < n; i++) std::memcpy(blob.data() + off[i], requests[i].hash, len[i]);
  check(cbft_bls_sign_batch(engine_->ctx(), signer_table_, nullptr, blob.data(), off.data(), len.data(), n, out.data()),
        "cbft_bls_sign_batch");
  for (size_t i = 0; i < n; i++) std::memcpy(requests[i].out, out.data() + 37 * i, 37);
}

// ------------------------------------------------------------------------------ key generation
using Scalar = std::array<uint8_t, 32>;

// r, the order of G1 / G2, big-endian
static const Scalar kGroupOrder = {0x25, 0x23, 0x64, 0x82, 0x40, 0x00, 0x00, 0x01, 0xba, 0x34, 0x4d,
                                   0x80, 0x00, 0x00, 0x00, 0x07, 0xff, 0x9f, 0x80, 0x00, 0x00, 0x00,
                                   0x00, 0x10, 0xa1, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x0d};

size_t keygenBatchMin() {  // read at every call: a keygen is rare, and tests switch it
  const char* e = std::getenv("CBFT_BLS_KEYGEN_BATCH_MIN");
  const long long x = e ? std::atoll(e) : 0;
  return x > 0 ? (size_t)x : (size_t)CBFT_BLS_KEYGEN_BATCH_MIN_DEFAULT;
}

bool scalarInRange(const Scalar& be) {
  unsigned any = 0;
  int lt = 0;  // the first differing byte decides; no early exit on a secret
  for (size_t i = 0; i < 32; i++) {
    any |= be[i];
    const int d = (int)be[i] - (int)kGroupOrder[i];
    lt = lt ? lt : d;
  }
  return any != 0 && lt < 0;
}

void sampleScalar(Scalar& out) {
  for (;;) {
    if (RAND_bytes(out.data(), 32) != 1) throw std::runtime_error("BLS keygen: RAND_bytes failed");
    out[0] &= 0x3f;  // r has 254 bits: more than half of the draws are kept
    if (scalarInRange(out)) return;
  }
}

static void wipeScalars(std::vector<Scalar>& v) {
  if (!v.empty()) OPENSSL_cleanse(v.data(), v.size() * sizeof(Scalar));
}

BlsThresholdKeygenBase::BlsThresholdKeygenBase(NumSharesType numSigners) : num_(numSigners) {
  if (numSigners < 1 || numSigners > MAX_NUM_OF_SHARES)
    throw std::invalid_argument("BLS keygen: need 1 <= numSigners <= 2048");
  skShares_.resize((size_t)numSigners + 1);
  pkShares_.resize((size_t)numSigners + 1);
  engine_ = BlsEngine::get();
}

void BlsThresholdKeygenBase::setKeys(const std::vector<Scalar>& scalars, const uint8_t* keys65, const uint8_t* ok) {
  for (size_t i = 0; i < scalars.size(); i++)
    if (!ok[i]) throw std::runtime_error("BLS keygen: a key's scalar is 0 mod r");
  sk_ = BlsSecretKey(scalars[0]);
  pk_ = BlsPublicKey(toHex(keys65, 65));
  for (size_t i = 1; i < scalars.size(); i++) {
    skShares_[i] = BlsSecretKey(scalars[i]);
    pkShares_[i] = BlsPublicKey(toHex(keys65 + 65 * i, 65));
  }
}

void BlsThresholdKeygenBase::deriveKeys(std::vector<Scalar>& scalars) {
  const size_t m = scalars.size();
  std::vector<uint8_t> keys(65 * m), ok(m, 0);
  if (m >= keygenBatchMin()) {
    check(cbft_bls_public_key_batch(engine_->ctx(), scalars[0].data(), m, keys.data(), ok.data()),
          "cbft_bls_public_key_batch");
  } else {
    for (size_t i = 0; i < m; i++) {
      const int rc = cbft_bls_public_key(engine_->ctx(), scalars[i].data(), &keys[65 * i]);
      if (rc != CBFT_EINVAL) check(rc, "cbft_bls_public_key");  // CBFT_EINVAL: the scalar is 0 mod r
      ok[i] = rc == CBFT_OK;
    }
  }
  setKeys(scalars, keys.data(), ok.data());
}

BlsThresholdKeygen::BlsThresholdKeygen(NumSharesType reqSigners, NumSharesType numSigners)
    : BlsThresholdKeygenBase(numSigners) {
  if (reqSigners < 1 || reqSigners > numSigners)
    throw std::invalid_argument("BLS keygen: need 1 <= reqSigners <= numSigners");
  std::vector<Scalar> c((size_t)reqSigners);
  for (auto& x : c) sampleScalar(x);
  try {
    deal(reqSigners, c);
  } catch (...) {
    wipeScalars(c);
    throw;
  }
  wipeScalars(c);
}

BlsThresholdKeygen::BlsThresholdKeygen(NumSharesType reqSigners, NumSharesType numSigners,
                                       const std::vector<Scalar>& coefficients)
    : BlsThresholdKeygenBase(numSigners) {
  if (reqSigners < 1 || reqSigners > numSigners || coefficients.size() != (size_t)reqSigners)
    throw std::invalid_argument("BLS keygen: need 1 <= reqSigners <= numSigners and reqSigners coefficients");
  std::vector<Scalar> c(coefficients);
  try {
    deal(reqSigners, c);
  } catch (...) {
    wipeScalars(c);
    throw;
  }
  wipeScalars(c);
}

// f(i) mod r for i = 1 .. n on the host (below the crossover): Horner with OpenSSL's constant-time flag set
static void dealOnHost(const std::vector<Scalar>& c, std::vector<Scalar>& scalars) {
  BN_CTX* bctx = BN_CTX_new();
  BIGNUM* r = BN_bin2bn(kGroupOrder.data(), 32, nullptr);
  BIGNUM* acc = BN_new();
  BIGNUM* x = BN_new();
  BIGNUM* cj = BN_new();
  bool good = bctx && r && acc && x && cj;
  if (good) {
    BN_set_flags(acc, BN_FLG_CONSTTIME);
    BN_set_flags(cj, BN_FLG_CONSTTIME);
  }
  for (size_t i = 0; good && i < scalars.size(); i++) {  // i = 0: f(0) = c_0 mod r
    good = BN_set_word(x, (BN_ULONG)i) == 1;
    BN_zero(acc);
    for (size_t j = c.size(); good && j-- > 0;) {
      good = BN_bin2bn(c[j].data(), 32, cj) != nullptr && BN_mod_mul(acc, acc, x, r, bctx) == 1 &&
             BN_mod_add(acc, acc, cj, r, bctx) == 1;
    }
    good = good && BN_bn2binpad(acc, scalars[i].data(), 32) == 32;
  }
  BN_clear_free(acc);
  BN_clear_free(cj);
  BN_free(x);
  BN_free(r);
  BN_CTX_free(bctx);
  if (!good) throw std::runtime_error("BLS keygen: host dealing failed");
}

void BlsThresholdKeygen::deal(NumSharesType reqSigners, std::vector<Scalar>& c) {
  const size_t n = (size_t)num_, m = n + 1;
  std::vector<Scalar> scalars(m);
  try {
    if (m >= keygenBatchMin()) {
      std::vector<uint8_t> keys(65 * m), ok(m, 0);
      const int rc = cbft_bls_keygen_threshold(engine_->ctx(), c[0].data(), (uint32_t)reqSigners, (uint32_t)n,
                                               scalars[1].data(), &keys[65], keys.data(), ok.data());
      check(rc, "cbft_bls_keygen_threshold");
      {  // the group secret is c_0 mod r = f(0)
        std::vector<Scalar> c0(1, c[0]), s0(1);
        dealOnHost(c0, s0);
        scalars[0] = s0[0];
        wipeScalars(c0);
        wipeScalars(s0);
      }
      setKeys(scalars, keys.data(), ok.data());
    } else {
      dealOnHost(c, scalars);
      deriveKeys(scalars);
    }
  } catch (...) {
    wipeScalars(scalars);
    throw;
  }
  wipeScalars(scalars);
}

BlsMultisigKeygen::BlsMultisigKeygen(NumSharesType numSigners) : BlsThresholdKeygenBase(numSigners) {
  std::vector<Scalar> s((size_t)numSigners);
  for (auto& x : s) sampleScalar(x);
  try {
    sum(s);
  } catch (...) {
    wipeScalars(s);
    throw;
  }
  wipeScalars(s);
}

BlsMultisigKeygen::BlsMultisigKeygen(NumSharesType numSigners, const std::vector<Scalar>& secrets)
    : BlsThresholdKeygenBase(numSigners) {
  if (secrets.size() != (size_t)numSigners) throw std::invalid_argument("BLS keygen: need numSigners secrets");
  for (const auto& x : secrets)
    if (!scalarInRange(x)) throw std::invalid_argument("BLS keygen: a secret outside [1, r)");
  std::vector<Scalar> s(secrets);
  try {
    sum(s);
  } catch (...) {
    wipeScalars(s);
    throw;
  }
  wipeScalars(s);
}

// acc = (acc + x) mod r for acc, x < r, big-endian bytes; the subtraction of r by a mask
static void addModOrder(Scalar& acc, const Scalar& x) {
  unsigned carry = 0;
  for (int i = 31; i >= 0; i--) {
    const unsigned v = (unsigned)acc[(size_t)i] + x[(size_t)i] + carry;
    acc[(size_t)i] = (uint8_t)v;
    carry = v >> 8;
  }  // r < 2^254: no carry out
  Scalar t;
  int borrow = 0;
  for (int i = 31; i >= 0; i--) {
    const int v = (int)acc[(size_t)i] - (int)kGroupOrder[(size_t)i] - borrow;
    t[(size_t)i] = (uint8_t)v;
    borrow = v < 0;
  }
  const uint8_t keep = (uint8_t)(0 - (unsigned)(1 - borrow));  // no borrow: acc >= r, the difference stands
  for (size_t i = 0; i < 32; i++) acc[i] = (uint8_t)((t[i] & keep) | (acc[i] & (uint8_t)~keep));
  OPENSSL_cleanse(t.data(), t.size());
}

void BlsMultisigKeygen::sum(std::vector<Scalar>& secrets) {
  std::vector<Scalar> scalars((size_t)num_ + 1);
  scalars[0].fill(0);
  for (size_t i = 0; i < secrets.size(); i++) {
    scalars[i + 1] = secrets[i];
    addModOrder(scalars[0], secrets[i]);
  }
  try {
    deriveKeys(scalars);
  } catch (...) {
    wipeScalars(scalars);
    throw;
  }
  wipeScalars(scalars);
}

// ------------------------------------------------------------------------------ factory
std::unique_ptr<BlsThresholdKeygenBase> BlsThresholdFactory::newKeygen(NumSharesType reqSigners,
                                                                       NumSharesType numSigners) const {
  if (multisigFor(reqSigners, numSigners)) return std::unique_ptr<BlsThresholdKeygenBase>(new BlsMultisigKeygen(numSigners));
  return std::unique_ptr<BlsThresholdKeygenBase>(new BlsThresholdKeygen(reqSigners, numSigners));
}

IThresholdVerifier* BlsThresholdFactory::newVerifier(ShareID reqSigners, ShareID numSigners, const char* publicKeyStr,
                                                     const std::vector<std::string>& verifKeysStr) const {
  if (numSigners < 1 || verifKeysStr.size() != (size_t)numSigners + 1)
    throw std::invalid_argument("BLS factory: need numSigners + 1 verification key strings (entry 0 unused)");
  const std::vector<std::string> vks(verifKeysStr.begin() + 1, verifKeysStr.end());
  if (multisigFor(reqSigners, numSigners)) return new BlsMultisigVerifier(reqSigners, numSigners, vks);
  return new BlsThresholdVerifier(publicKeyStr ? std::string(publicKeyStr) : std::string(), reqSigners, numSigners, vks);
}

IThresholdSigner* BlsThresholdFactory::newSigner(ShareID id, const char* secretKeyStr) const {
  if (!secretKeyStr) throw std::invalid_argument("BLS factory: no secret key");
  return new BlsThresholdSigner(id, secretKeyStr);
}

std::tuple<std::vector<IThresholdSigner*>, IThresholdVerifier*> BlsThresholdFactory::newRandomSigners(
    NumSharesType reqSigners, NumSharesType numSigners) const {
  std::unique_ptr<BlsThresholdKeygenBase> keygen(newKeygen(reqSigners, numSigners));
  std::vector<IThresholdSigner*> signers((size_t)numSigners + 1, nullptr);  // indexed from 1
  std::vector<std::string> vks((size_t)numSigners + 1);
  IThresholdVerifier* verifier = nullptr;
  try {
    for (ShareID i = 1; i <= numSigners; i++) {
      vks[(size_t)i] = keygen->getShareVerificationKey(i).toString();
      // the key the keygen derived is handed over: no second sk * g2 per signer
      signers[(size_t)i] = new BlsThresholdSigner(i, keygen->getShareSecretKey(i).toString(), vks[(size_t)i]);
    }
    const std::string pk = keygen->getPublicKey().toString();
    verifier = newVerifier(reqSigners, numSigners, pk.c_str(), vks);
  } catch (...) {
    for (auto* s : signers) delete s;
    throw;
  }
  return std::make_tuple(signers, verifier);
}

std::pair<std::unique_ptr<IShareSecretKey>, std::unique_ptr<IShareVerificationKey>> BlsThresholdFactory::newKeyPair() const {
  if (!useMultisig_) throw std::runtime_error("BlsThresholdFactory::newKeyPair allowed for multisig only");
  BlsMultisigKeygen keygen(1);
  return std::make_pair(std::unique_ptr<IShareSecretKey>(new BlsSecretKey(keygen.getShareSecretKey(1))),
                        std::unique_ptr<IShareVerificationKey>(new BlsPublicKey(keygen.getShareVerificationKey(1))));
}

}  // namespace Hip
}  // namespace BLS
