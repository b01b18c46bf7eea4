// BLS BN-P254 threshold signatures over libcbft_hipcrypto: the objects a Cryptosystem subclass
// returns from createThresholdVerifier / createThresholdSigner (ThresholdSignaturesTypes.h:280,294
// of the reference), with the reference's class names and behaviour:
//
//   BlsThresholdVerifier   threshsign/src/bls/relic/BlsThresholdVerifier.cpp:26-96
//   BlsMultisigVerifier    threshsign/src/bls/relic/BlsMultisigVerifier.cpp:27-105
//   BlsThresholdAccumulator, BlsMultisigAccumulator, and the k = n - 1 "almost multisig" case
//                          ThresholdAccumulatorBase.cpp:14-147, BlsAccumulatorBase.cpp:33-84,
//                          BlsThresholdAccumulator.cpp:29-55, BlsMultisigAccumulator.cpp:30-65,
//                          BlsAlmostMultisigAccumulator.cpp:28-46
//   BlsThresholdSigner     threshsign/src/bls/relic/BlsThresholdSigner.cpp:25-47
//   BlsThresholdKeygen, BlsMultisigKeygen, BlsThresholdFactory
//                          BlsThresholdKeygen.cpp:28-50, BlsMultisigKeygen.cpp:22-40,
//                          BlsThresholdFactory.cpp:41-119 (what Cryptosystem::createThresholdFactory returns)
//
// Difference by design: where the reference verifies pending shares one pairing pair at a time
// (ThresholdAccumulatorBase::verifyPendingShares), this accumulator verifies all pending shares
// in one GPU launch and then applies the reference's walk (id order, stop at reqSigners, the
// rest of the invalid ones reported), so valid/invalid sets are identical.
//
// Key encodings: PK and vk_i are 65-byte compressed G2 points as hex strings (130 characters,
// ThresholdSignaturesTypes.cpp:220-228); share secret keys are decimal strings
// (BlsSecretKey.h:37, BNT::toString base 10).  The G2/G1 encodings are RELIC's (Montgomery-form
// y parity), pinned by the reference's own key files (tests/golden/relic_bls_keys.json).
#pragma once

#include <array>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "threshsign/IThresholdAccumulator.h"
#include "threshsign/IThresholdFactory.h"
#include "threshsign/IThresholdSigner.h"
#include "threshsign/IThresholdVerifier.h"
#include "threshsign/VectorOfShares.h"

namespace BLS {
namespace Hip {

class BlsEngine;  // per-process owner of a cbft_ctx (device from CBFT_DEVICE, default 0)

class BlsPublicKey : public IShareVerificationKey {
 public:
  BlsPublicKey() = default;
  explicit BlsPublicKey(const std::string& hex);  // throws std::invalid_argument if not 130 hex
  std::string toString() const override { return hex_; }
  const std::array<uint8_t, 65>& bytes() const { return raw_; }
  bool operator==(const BlsPublicKey& o) const { return raw_ == o.raw_; }

 private:
  std::string hex_;
  std::array<uint8_t, 65> raw_{};
};

class BlsSecretKey : public IShareSecretKey {
 public:
  BlsSecretKey() = default;                           // the number 0, toString() empty
  explicit BlsSecretKey(const std::string& decimal);  // throws std::invalid_argument
  explicit BlsSecretKey(const std::array<uint8_t, 32>& bigEndian);  // toString() is its decimal form
  ~BlsSecretKey() override;                           // wipes both copies
  std::string toString() const override { return dec_; }
  const std::array<uint8_t, 32>& bytes() const { return be_; }  // big-endian

 private:
  std::string dec_;
  std::array<uint8_t, 32> be_{};
};

// One check of BlsThresholdVerifier::verifyBatch.  signer == 0: sig is a 33-byte combined signature,
// ok = what verify(msg, msgLen, sig, sigLen) gives.  signer >= 1: sig is that signer's share, 37 bytes
// (id || point, the id must be the signer's) or the 33-byte point alone, ok = what an accumulator's
// share check gives (false for a signer outside [1, numSigners] or any other length).
struct BlsVerifyRequest {
  const char* msg;
  int msgLen;
  const char* sig;
  int sigLen;
  ShareID signer;
  bool ok;
};

// What verifyBatch hands to ONE cbft_bls_verify_batch call: the requests that pass the length and id
// checks (item j is request item[j]), identical messages stored once (msgOf).  Built without the GPU.
struct BlsVerifyPlan {
  std::vector<uint32_t> item, keyIdx, msgOf, msgLen;
  std::vector<uint64_t> msgOff;
  std::vector<uint8_t> sig33, blob;
};

// Smallest BlsThresholdVerifier::verifyBatch that runs as ONE cbft_bls_verify_batch call
// ($CBFT_BLS_VERIFY_BATCH_MIN overrides); smaller batches loop the lone calls (cbft_bls_verify,
// cbft_bls_verify_shares).  The measured crossover of one batch call against n lone cbft_bls_verify
// calls, host arrays in to verdicts out.
#define CBFT_BLS_VERIFY_BATCH_MIN_DEFAULT 2

class BlsThresholdVerifier : public IThresholdVerifier {
 public:
  // vkHex: numSigners share verification keys vk_1..vk_n (the reference's vector has a dummy
  // entry 0; here index 0 is vk_1).
  BlsThresholdVerifier(const std::string& pkHex, NumSharesType reqSigners, NumSharesType numSigners,
                       const std::vector<std::string>& vkHex);
  ~BlsThresholdVerifier() override;

  IThresholdAccumulator* newAccumulator(bool withShareVerification) const override;
  bool verify(const char* msg, int msgLen, const char* sig, int sigLen) const override;
  // The batch form of verify and of the accumulators' share check for the certificates and shares of
  // many sequence numbers: every request's ok is set.  batchMin() requests or more run as one
  // cbft_bls_verify_batch call, fewer as lone calls; the verdicts are the same.
  virtual void verifyBatch(std::vector<BlsVerifyRequest>& requests) const;
  static size_t batchMin();
  // the requests that need a pairing, packed for one call; the others get ok = false here
  static void planBatch(std::vector<BlsVerifyRequest>& requests, NumSharesType numSigners, BlsVerifyPlan& plan);
  int requiredLengthForSignedData() const override { return 33; }
  const IPublicKey& getPublicKey() const override { return pk_; }
  const IShareVerificationKey& getShareVerificationKey(ShareID signer) const override;

  NumSharesType getNumRequiredShares() const { return req_; }
  NumSharesType getNumTotalShares() const { return num_; }
  uint32_t keysetId() const { return keyset_; }
  const std::shared_ptr<BlsEngine>& engine() const { return engine_; }

 protected:
  BlsPublicKey pk_;
  std::vector<BlsPublicKey> vks_;
  NumSharesType req_, num_;
  std::shared_ptr<BlsEngine> engine_;
  uint32_t keyset_ = 0;
};

// What the k-of-n verifyBatch hands to ONE cbft_bls_verify_multisig_batch call: the signer == 0 requests
// that pass verify()'s host-side rules (length, at least reqSigners signers, no id above numSigners; item j
// is request item[j]), identical signer bitmaps stored once (setOf) and identical messages stored once
// (msgOf).  Built without the GPU.
struct BlsMultisigPlan {
  std::vector<uint32_t> item, setOf, msgOf, msgLen;
  std::vector<uint64_t> msgOff;
  std::vector<uint8_t> sig33, sets, blob;
};

// Smallest number of k-of-n certificates that BlsMultisigVerifier::verifyBatch runs as ONE
// cbft_bls_verify_multisig_batch call ($CBFT_BLS_MULTISIG_BATCH_MIN overrides); fewer loop
// cbft_bls_verify_multisig.  The measured crossover of one batch call against n lone calls, host arrays in
// to verdicts out.
#define CBFT_BLS_MULTISIG_BATCH_MIN_DEFAULT 3

class BlsMultisigVerifier : public BlsThresholdVerifier {
 public:
  // PK is the sum of the vk_i (BlsMultisigVerifier.cpp:33-38); pkHex is not needed.
  BlsMultisigVerifier(NumSharesType reqSigners, NumSharesType numSigners, const std::vector<std::string>& vkHex);
  IThresholdAccumulator* newAccumulator(bool withShareVerification) const override;
  // n-of-n: 33 bytes; otherwise 33 + 256 (signer bitmap) (BlsMultisigVerifier.cpp:67-73)
  int requiredLengthForSignedData() const override;
  // throws std::runtime_error on a wrong-size k-of-n signature (BlsMultisigVerifier.cpp:77)
  bool verify(const char* msg, int msgLen, const char* sig, int sigLen) const override;
  // n-of-n: 33-byte signatures go through the batch under the summed key.  k-of-n: a signature carries
  // its signer bitmap and is checked under its own key sum: multisigBatchMin() such requests or more run as
  // one cbft_bls_verify_multisig_batch call, fewer through verify() one by one; the verdicts are the same
  // (ok = false instead of verify()'s exception for a wrong size).  Shares still run as one batch.
  void verifyBatch(std::vector<BlsVerifyRequest>& requests) const override;
  static size_t multisigBatchMin();
  // the signer == 0 requests that need a pairing, packed for one call, with ok = false for all of them;
  // requests with signer != 0 are left alone
  static void planMultisigBatch(std::vector<BlsVerifyRequest>& requests, NumSharesType reqSigners,
                                NumSharesType numSigners, BlsMultisigPlan& plan);
};

struct BlsCombineInput;

// Accumulator state machine of ThresholdAccumulatorBase (pending / valid / invalid shares).
class BlsAccumulatorBase : public IThresholdAccumulator {
 public:
  BlsAccumulatorBase(const BlsThresholdVerifier& v, NumSharesType reqSigners, bool withShareVerification);
  int add(const char* sigShareWithId, int len) override;
  void setExpectedDigest(const unsigned char* msg, int len) override;
  bool hasShareVerificationEnabled() const override { return verify_; }
  int getNumValidShares() const override;
  std::set<ShareID> getInvalidShareIds() const override { return invalid_; }
  int addNumById(ShareID signer, const uint8_t* share33);
  // What getFullSignedData combines, for combineBatch: the valid shares as 37-byte records in id order,
  // whether they are summed plainly (multisig), and the signer bitmap that follows the signature
  // (k-of-n multisig: 256 bytes; otherwise empty)
  void combineInput(BlsCombineInput& in) const;
  const BlsThresholdVerifier& verifier() const { return v_; }

 protected:
  virtual bool multisig() const = 0;
  using Share = std::array<uint8_t, 33>;
  bool hasExpectedDigest() const { return !digest_.empty(); }
  void verifyPendingShares();
  // valid shares as 37-byte (id || point) records in id order
  std::vector<uint8_t> validRecords() const;

  const BlsThresholdVerifier& v_;
  NumSharesType req_, num_;
  bool verify_;
  std::vector<uint8_t> digest_;
  std::vector<Share> pending_, valid_;
  VectorOfShares pendingBits_, validBits_;
  std::set<ShareID> invalid_;
};

class BlsThresholdAccumulator : public BlsAccumulatorBase {
 public:
  using BlsAccumulatorBase::BlsAccumulatorBase;
  // sum lambda_i sigma_i over the valid shares -> 33 bytes (throws std::runtime_error if
  // threshSigLen < 33 or a share does not decode)
  void getFullSignedData(char* outThreshSig, int threshSigLen) override;

 protected:
  bool multisig() const override { return false; }
};

class BlsMultisigAccumulator : public BlsAccumulatorBase {
 public:
  using BlsAccumulatorBase::BlsAccumulatorBase;
  // sum sigma_i -> 33 bytes, || 256-byte signer bitmap when reqSigners != numSigners
  void getFullSignedData(char* outThreshSig, int threshSigLen) override;

 protected:
  bool multisig() const override { return true; }
};

// One certificate to combine in combineBatch: out receives what acc->getFullSignedData(out, outLen)
// writes (33 bytes, 33 + 256 for a k-of-n multisig accumulator); ok = false where that call would throw
// (out too short, a share that does not decode), and out is then left as it was.
struct BlsCombineRequest {
  IThresholdAccumulator* acc;
  char* out;
  int outLen;
  bool ok;
};

// An accumulator's state as combineBatch reads it (BlsAccumulatorBase::combineInput); usable = false
// for a null pointer or an accumulator of another implementation.
struct BlsCombineInput {
  bool usable = false;
  bool multisig = false;
  std::vector<uint8_t> records;  // 37 bytes per valid share, id order
  std::vector<uint8_t> signers;  // what follows the signature in out
};

// What combineBatch hands to ONE cbft_bls_combine_batch call: the requests that pass the buffer checks
// and hold at least one share (certificate j is request item[j], its shares certOff[j] .. certOff[j + 1]
// of shares37).  Built without the GPU.
struct BlsCombinePlan {
  std::vector<uint32_t> item;
  std::vector<uint64_t> certOff;
  std::vector<uint8_t> shares37;
  bool multisig = false;
};

// Smallest combineBatch that runs as ONE cbft_bls_combine_batch call ($CBFT_BLS_COMBINE_BATCH_MIN
// overrides); smaller ones loop getFullSignedData (cbft_bls_combine).  The measured crossover of one
// batch call against m lone calls at k = 5, host arrays in to host arrays out.
#define CBFT_BLS_COMBINE_BATCH_MIN_DEFAULT 5

// The batch form of getFullSignedData over the accumulators of ONE verifier (a collector's window of
// sequence numbers, the certificates of a view change): every request's ok is set and every out that
// is ok holds the bytes the lone call writes.  combineBatchMin() requests or more run as one
// cbft_bls_combine_batch call, fewer as lone calls; the outputs are the same.  Throws
// std::invalid_argument when the accumulators are of different verifiers.
void combineBatch(std::vector<BlsCombineRequest>& requests);
size_t combineBatchMin();
// Packing, offsets and refusals: requests that need no device (no buffer, a short one, an unusable
// accumulator: ok = false; no valid share: the identity, ok = true) are answered here, the others packed
// for one call.  in[i] is request i's accumulator.  Throws std::invalid_argument on mixed kinds.
void planCombine(const std::vector<BlsCombineInput>& in, std::vector<BlsCombineRequest>& requests, BlsCombinePlan& plan);

// One share to sign in BlsThresholdSigner::signBatch: out receives 37 bytes (outLen >= 37).
struct BlsSignRequest {
  const char* hash;
  int hashLen;
  char* out;
  int outLen;
};

// Smallest BlsThresholdSigner::signBatch that signs in ONE cbft_bls_sign_batch call
// ($CBFT_BLS_SIGN_BATCH_MIN overrides); smaller batches loop cbft_bls_sign.  Both run on the GPU (the
// product path has no CPU signer).  The measured crossover of one batch call against n lone calls,
// host arrays in to host arrays out.
#define CBFT_BLS_SIGN_BATCH_MIN_DEFAULT 8

class BlsThresholdSigner : public IThresholdSigner {
 public:
  // vkHex empty: the verification key is derived from the secret key on the GPU (sk * g2), as
  // the reference's constructor does (BlsThresholdSigner.cpp:25)
  BlsThresholdSigner(ShareID id, const std::string& secretKeyDecimal, const std::string& vkHex = "");
  int requiredLengthForSignedData() const override { return 37; }
  // outSig = 4-byte big-endian id || sk * H(hash); throws std::runtime_error if outSigLen < 37
  void signData(const char* hash, int hashLen, char* outSig, int outSigLen) override;
  // The batch form of signData for the shares of several sequence numbers in flight: every out gets
  // the bytes signData gives for its hash.  The key is registered in a signer table of the engine at
  // the first batch of batchMin() requests or more.  Throws as signData does, before anything is signed.
  void signBatch(const std::vector<BlsSignRequest>& requests);
  static size_t batchMin();
  ~BlsThresholdSigner() override;
  BlsThresholdSigner(const BlsThresholdSigner&) = delete;
  BlsThresholdSigner& operator=(const BlsThresholdSigner&) = delete;
  const IShareSecretKey& getShareSecretKey() const override { return sk_; }
  const IShareVerificationKey& getShareVerificationKey() const override { return vk_; }

 private:
  ShareID id_;
  BlsSecretKey sk_;
  BlsPublicKey vk_;
  std::shared_ptr<BlsEngine> engine_;
  std::mutex table_mu_;        // guards the registration below (concurrent first batches)
  uint32_t signer_table_ = 0;  // one-key table of the engine's context, loaded by the first GPU batch
};

// ------------------------------------------------------------------------------ key generation
// Smallest number of keys (shares plus the group key) that a keygen derives with ONE batch call
// (cbft_bls_keygen_threshold, cbft_bls_public_key_batch; $CBFT_BLS_KEYGEN_BATCH_MIN overrides, default
// CBFT_BLS_KEYGEN_BATCH_MIN_DEFAULT of cbft_hipcrypto.h); fewer loop the lone cbft_bls_public_key, with the
// shares dealt on the host.  The keys are the same.  The measured crossover.
size_t keygenBatchMin();
// 32 big-endian bytes uniform in [1, r): OpenSSL RAND_bytes masked to 254 bits, drawn again while the
// value is 0 or >= r.  Throws std::runtime_error if the generator fails.
void sampleScalar(std::array<uint8_t, 32>& out);
bool scalarInRange(const std::array<uint8_t, 32>& bigEndian);  // 1 <= value < r

// The reference keygens' accessors (IThresholdKeygen<SK, PK>): group secret and PK, share secret keys and
// share verification keys indexed from 1 (entry 0 of the vectors is unused).
class BlsThresholdKeygenBase {
 public:
  virtual ~BlsThresholdKeygenBase() = default;
  NumSharesType getNumSigners() const { return num_; }
  const BlsSecretKey& getSecretKey() const { return sk_; }
  const BlsPublicKey& getPublicKey() const { return pk_; }
  const BlsSecretKey& getShareSecretKey(ShareID i) const { return skShares_.at((size_t)i); }
  const BlsPublicKey& getShareVerificationKey(ShareID i) const { return pkShares_.at((size_t)i); }
  const std::vector<BlsSecretKey>& getShareSecretKeys() const { return skShares_; }
  const std::vector<BlsPublicKey>& getShareVerificationKeys() const { return pkShares_; }

 protected:
  explicit BlsThresholdKeygenBase(NumSharesType numSigners);
  // scalars[0] = the group secret, scalars[i] = share i -> sk_, skShares_, pk_, pkShares_ (one batch call
  // from keygenBatchMin() keys on, else lone calls); throws std::runtime_error if a scalar is 0 mod r
  void deriveKeys(std::vector<std::array<uint8_t, 32>>& scalars);
  void setKeys(const std::vector<std::array<uint8_t, 32>>& scalars, const uint8_t* keys65, const uint8_t* ok);

  NumSharesType num_;
  BlsSecretKey sk_;
  BlsPublicKey pk_;
  std::vector<BlsSecretKey> skShares_;
  std::vector<BlsPublicKey> pkShares_;
  std::shared_ptr<BlsEngine> engine_;
};

// Shamir dealing: sk_i = f(i) for a polynomial of degree reqSigners - 1 over Fr, vk_i = sk_i * g2,
// PK = f(0) * g2.  1 <= reqSigners <= numSigners <= 2048 (std::invalid_argument).
class BlsThresholdKeygen : public BlsThresholdKeygenBase {
 public:
  BlsThresholdKeygen(NumSharesType reqSigners, NumSharesType numSigners);  // coefficients from sampleScalar
  // the reqSigners coefficients c_0 .. c_{k-1} given (32 bytes big-endian each, reduced mod r): for tests
  BlsThresholdKeygen(NumSharesType reqSigners, NumSharesType numSigners,
                     const std::vector<std::array<uint8_t, 32>>& coefficients);

 private:
  void deal(NumSharesType reqSigners, std::vector<std::array<uint8_t, 32>>& coefficients);
};

// numSigners independent secrets, group secret = their sum mod r, PK = that sum * g2 (= the sum of the vk_i).
class BlsMultisigKeygen : public BlsThresholdKeygenBase {
 public:
  explicit BlsMultisigKeygen(NumSharesType numSigners);  // secrets from sampleScalar
  BlsMultisigKeygen(NumSharesType numSigners, const std::vector<std::array<uint8_t, 32>>& secrets);  // for tests

 private:
  void sum(std::vector<std::array<uint8_t, 32>>& secrets);
};

// The reference's BlsThresholdFactory without its curve parameter (BN-P254 is the only curve).  As
// Cryptosystem does (forceMultisig_, ThresholdSignaturesTypes.cpp:31), reqSigners == numSigners takes the
// multisig scheme whatever the flag says.
class BlsThresholdFactory : public IThresholdFactory {
 public:
  explicit BlsThresholdFactory(bool useMultisig = false) : useMultisig_(useMultisig) {}
  std::unique_ptr<BlsThresholdKeygenBase> newKeygen(NumSharesType reqSigners, NumSharesType numSigners) const;
  // publicKeyStr: 130 hex characters (ignored by the multisig scheme); verifKeysStr[1 .. numSigners] likewise
  IThresholdVerifier* newVerifier(ShareID reqSigners, ShareID numSigners, const char* publicKeyStr,
                                  const std::vector<std::string>& verifKeysStr) const override;
  IThresholdSigner* newSigner(ShareID id, const char* secretKeyStr) const override;  // decimal secret key
  std::tuple<std::vector<IThresholdSigner*>, IThresholdVerifier*> newRandomSigners(
      NumSharesType reqSigners, NumSharesType numSigners) const override;
  // multisig only, as the reference's (std::runtime_error otherwise)
  std::pair<std::unique_ptr<IShareSecretKey>, std::unique_ptr<IShareVerificationKey>> newKeyPair() const override;
  bool multisigFor(NumSharesType reqSigners, NumSharesType numSigners) const {
    return useMultisig_ || reqSigners == numSigners;
  }

 private:
  bool useMultisig_;
};

}  // namespace Hip
}  // namespace BLS
