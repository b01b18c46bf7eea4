// GPU-backed implementations of the reference's signature plugin interface
// (concord::util::crypto::IVerifier / ISigner, util/include/crypto_utils.hpp:41-55) over
// libcbft_hipcrypto, in namespace concord::hip so that nothing here redefines a reference symbol:
// this header and hip_verifiers.cpp / hip_rsa.cpp / hip_ecdsa.cpp compile against the reference's own
// crypto_utils.hpp (tests/test_reference_boundary.py) or, where the reference cannot be built,
// against the restatement in ref_mirror/include/crypto_utils.hpp.
//
//   HipEdDSAVerifier : IVerifier   Ed25519 (RFC 8032 as OpenSSL 3.0.2 EVP_DigestVerify accepts it,
//                                  util/src/openssl_crypto.cpp:229-253 idiom); the reference has no
//                                  Ed25519, so semantics are pinned by the
//                                  golden vectors
//   HipRSAVerifier : IVerifier     RSASS<PKCS1v15, SHA256> with Crypto++ 8.2.0 semantics
//                                  (util/src/crypto_utils.cpp:101-117), 2048-bit moduli
//   HipECDSAVerifier : IVerifier   ECDSA / SHA-256 (Crypto++ ECDSA<ECP, SHA256>, crypto_utils.cpp:34-64):
//                                  secp256k1 and prime256v1 keys on the GPU with OpenSSL 3.0.2's verdicts,
//                                  keys on other curves on the host OpenSSL
//   HipP256PublicKey               ECDSA P-256 / SHA-256 with DER signatures, the shape of
//                                  concord::util::openssl_utils::AsymmetricPublicKey (openssl_crypto.cpp)
//   HipP256PrivateKey              its private half (AsymmetricPrivateKey): RFC 6979 signatures in DER, sign() with
//                                  the GPU's lane code on the host, signBatch() on the GPU
//   EdDSASigner : ISigner          Ed25519 signing: sign() on the host OpenSSL (one signature is
//                                  latency-bound on any device); signBatch() on the GPU from
//                                  CBFT_SIGN_GPU_MIN requests up (the pre-processing path signs one
//                                  result hash per request, PreProcessReplyMsg.cpp:142-160), byte for
//                                  byte the signatures sign() gives
//   HipRSASigner : RSASigner       the reference's RSA signer with a batch side: sign() is the
//                                  reference's own; signBatch() signs on the GPU (CRT, constant time,
//                                  every signature checked before release) from
//                                  CBFT_RSA_SIGN_GPU_MIN requests up, byte for byte what sign() gives
//   makeVerifier / makeSigner      the branch SigManager needs where it hard-codes RSAVerifier /
//                                  RSASigner (SigManager.cpp:138,146,255)
//   verifyBatch                    the batch side-API: many (verifier, data, sig) triples, one GPU
//                                  launch per algorithm, verdicts identical to verify() on each
//
// Contract kept from the reference: verify() returns false for any bad signature and never throws
// (openssl_crypto.cpp:247-253); a GPU failure is reported as false and counted
// (engineStats().gpu_errors), never thrown into the pool threads that call verify().  Key parsing
// throws std::invalid_argument.
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "crypto_utils.hpp"
#include "latency_histogram.hpp"

namespace concord::hip {

using concord::util::crypto::ISigner;
using concord::util::crypto::IVerifier;
using concord::util::crypto::KeyFormat;

class Ed25519Engine;  // per-process owner of the cbft_ctx and of the device key table
class RsaEngine;      // the same for RSA keys

// One (verifier, message, signature) triple of a batch.  Pointers are borrowed.
struct VerifyRequest {
  const IVerifier* verifier;
  const char* data;
  size_t dataLength;
  const char* sig;
  size_t sigLength;
};

// One message of a signing batch: outSig receives signatureLength() bytes.  Pointers are borrowed.
struct SignRequest {
  const char* data;
  size_t dataLength;
  char* outSig;
};

// Smallest EdDSASigner::signBatch that goes to the GPU ($CBFT_SIGN_GPU_MIN overrides): the
// measured crossover of one cbft_ed25519_sign_batch call, host arrays in to host arrays out,
// against a loop of sign() on one core, rounded up to a power of two.
#define CBFT_SIGN_GPU_MIN_DEFAULT 64

// A registered Ed25519 key slot: copies share the slot, the last copy releases it (a released
// slot is reused by the next new key: rotated client keys do not grow the device table).
class Ed25519KeyRef {
 public:
  Ed25519KeyRef(std::shared_ptr<Ed25519Engine> engine, uint32_t index) : engine_(std::move(engine)), index_(index) {}
  Ed25519KeyRef(const Ed25519KeyRef& o);
  Ed25519KeyRef& operator=(const Ed25519KeyRef&) = delete;
  ~Ed25519KeyRef();
  uint32_t index() const { return index_; }
  Ed25519Engine& engine() const { return *engine_; }

 private:
  std::shared_ptr<Ed25519Engine> engine_;
  uint32_t index_;
};

class HipEdDSAVerifier : public IVerifier {
 public:
  // Raw 32-byte key or its SubjectPublicKeyInfo (RFC 8410), hex or PEM.  Throws
  // std::invalid_argument on a malformed key; a well-formed 32-byte string that is not a curve
  // point is accepted and every signature under it verifies false (as OpenSSL does).
  HipEdDSAVerifier(const std::string& str_pub_key, KeyFormat fmt);
  ~HipEdDSAVerifier() override;
  HipEdDSAVerifier(const HipEdDSAVerifier&) = default;

  bool verify(const std::string& data, const std::string& sig) const override;
  uint32_t signatureLength() const override { return 64; }
  std::string getPubKey() const override { return key_str_; }

  const uint8_t* rawKey() const { return raw_; }
  uint32_t engineKeyIndex() const { return key_.index(); }
  // Verifies every request whose verifier is a HipEdDSAVerifier in one GPU batch; out[i] =
  // verdict of reqs[i] (false for other verifier types).
  static void verifyBatch(const std::vector<VerifyRequest>& reqs, std::vector<bool>& out);

 private:
  std::string key_str_;
  uint8_t raw_[32];
  Ed25519KeyRef key_;
};

class HipRSAVerifier : public IVerifier {
 public:
  // X.509 SubjectPublicKeyInfo, hex DER (HexaDecimalStrippedFormat, as Crypto++'s
  // RSA::PublicKey::Save writes it) or PEM.  Throws std::invalid_argument unless it is a 2048-bit
  // RSA key with a public exponent < 2^32.
  HipRSAVerifier(const std::string& str_pub_key, KeyFormat fmt);
  ~HipRSAVerifier() override;
  HipRSAVerifier(const HipRSAVerifier&) = default;

  // Crypto++ VerifyMessage semantics: the signature is a big-endian integer of any length
  // (leading zero bytes are insignificant); more than 256 significant bytes is rejected (the
  // reference's callers check signatureLength() first, ClientRequestMsg.cpp:156).
  bool verify(const std::string& data, const std::string& sig) const override;
  uint32_t signatureLength() const override { return 256; }
  std::string getPubKey() const override { return key_str_; }

  uint32_t engineKeyIndex() const { return key_index_; }
  static void verifyBatch(const std::vector<VerifyRequest>& reqs, std::vector<bool>& out);

 private:
  std::string key_str_;
  uint32_t key_index_;
  std::shared_ptr<RsaEngine> engine_;
};

class EcdsaEngine;  // per-process owner of the cbft_ctx and of the device ECDSA key table

// Smallest number of secp256k1 items in one verifyBatch (or one verify(): 1) that goes to the GPU
// ($CBFT_ECDSA_GPU_MIN overrides): the measured crossover of one cbft_ecdsa_verify_batch call, host
// arrays in to bitmap out, against a one-thread loop of OpenSSL ECDSA_do_verify.
// Below it the items are verified on the host with OpenSSL, whose verdicts the GPU path reproduces.
#define CBFT_ECDSA_GPU_MIN_DEFAULT 32
// The same for prime256v1 (P-256) items ($CBFT_ECDSA_P256_GPU_MIN overrides), against a one-thread loop of
// OpenSSL's P-256 ECDSA_do_verify, which is several times faster than its secp256k1: 128
// (profiles/ecdsa_p256_verify.json "crossover").
#define CBFT_ECDSA_P256_GPU_MIN_DEFAULT 128

// ECDSA / SHA-256 in place of concord::util::crypto::ECDSAVerifier (Crypto++ ECDSA<ECP, SHA256>,
// util/include/crypto_utils.hpp:57-77).  Signatures are r || s, each as long as the group order
// (IEEE P1363, what Crypto++ reads and writes).  A secp256k1 key (the reference's default curve)
// registers with the process's key table and is verified on the GPU from gpuMinBatch() items per
// call up; a prime256v1 (P-256) key registers in a table of its own and goes to the GPU from
// gpuMinBatchP256() items up; a key on any other curve the host OpenSSL knows (KeyExchangeManager generates secp384r1
// keys) is verified with OpenSSL.
class HipECDSAVerifier : public IVerifier {
 public:
  // X.509 SubjectPublicKeyInfo of an EC key, hex DER or PEM.  Throws std::invalid_argument unless it
  // parses as an EC public key on a named curve.
  HipECDSAVerifier(const std::string& str_pub_key, KeyFormat fmt);
  ~HipECDSAVerifier() override;
  HipECDSAVerifier(const HipECDSAVerifier&) = delete;
  HipECDSAVerifier& operator=(const HipECDSAVerifier&) = delete;

  // false for any signature whose length is not signatureLength() (Crypto++ throws for a short
  // one; verify() here never throws on bad input), otherwise the ECDSA verdict.
  bool verify(const std::string& data, const std::string& sig) const override;
  uint32_t signatureLength() const override { return sig_len_; }
  std::string getPubKey() const override { return key_str_; }

  bool gpuCapable() const { return gpu_capable_; }
  uint32_t engineKeyIndex() const { return key_index_; }
  static size_t gpuMinBatch();
  static size_t gpuMinBatchP256();
  // CBFT_CURVE_* of a GPU-capable key (secp256k1 or prime256v1)
  int curve() const { return curve_; }
  // Verifies every request whose verifier is a HipECDSAVerifier: the secp256k1 ones in one GPU
  // batch when there are gpuMinBatch() or more of them, the prime256v1 ones in another when there are
  // gpuMinBatchP256() or more of them, everything else on the host; out[i] = verdict of reqs[i] (false
  // for other verifier types).
  static void verifyBatch(const std::vector<VerifyRequest>& reqs, std::vector<bool>& out);

 private:
  bool verifyHost(const char* data, size_t len, const char* sig, size_t sig_len) const;
  std::string key_str_;
  uint32_t sig_len_ = 0;
  bool gpu_capable_ = false;
  uint32_t key_index_ = 0;
  int curve_ = 0;         // CBFT_CURVE_* when gpu_capable_
  uint8_t pub_[64] = {0};  // X || Y of a GPU-capable key
  void* pkey_ = nullptr;  // EVP_PKEY* for the host path
  std::shared_ptr<EcdsaEngine> engine_;
  friend class HipP256PublicKey;
};

// ECDSA P-256 / SHA-256 public key in the shape of concord::util::openssl_utils::AsymmetricPublicKey
// (util/include/openssl_crypto.hpp): built from the serialised form "PUBLIC_KEY:secp256r1:<hex point>",
// verifies DER-encoded signatures.  A thin adapter: csrc/ecdsa_der.h turns the signature into r || s
// (anything but the canonical encoding is verdict false, as OpenSSL's ECDSA_verify has it), then the
// HipECDSAVerifier path for a prime256v1 key.
class HipP256PublicKey {
 public:
  // Throws std::invalid_argument unless `serialized` is PUBLIC_KEY:secp256r1: and a hex point on the curve.
  explicit HipP256PublicKey(const std::string& serialized);
  ~HipP256PublicKey();
  HipP256PublicKey(const HipP256PublicKey&) = delete;
  HipP256PublicKey& operator=(const HipP256PublicKey&) = delete;

  bool verify(const std::string& message, const std::string& der_signature) const;
  std::string serialize() const;  // PUBLIC_KEY:secp256r1:04<X><Y>, upper-case hex
  const HipECDSAVerifier& verifier() const { return *verifier_; }

  struct Request {
    const HipP256PublicKey* key;
    const char* data;
    size_t dataLength;
    const char* sig;  // DER
    size_t sigLength;
  };
  // out[i] = verdict of reqs[i]; the parsed signatures go through HipECDSAVerifier::verifyBatch together
  static void verifyBatch(const std::vector<Request>& reqs, std::vector<bool>& out);

 private:
  std::unique_ptr<HipECDSAVerifier> verifier_;
};

// Smallest HipP256PrivateKey::signBatch that goes to the GPU ($CBFT_ECDSA_P256_SIGN_GPU_MIN overrides): the
// crossover of one cbft_ecdsa_sign_batch call on a P-256 signer table, host arrays in to host arrays out,
// against the class's own host loop on one core, rounded up to a power of two
// (profiles/ecdsa_p256_sign.json "crossover").
#define CBFT_ECDSA_P256_SIGN_GPU_MIN_DEFAULT 16

// ECDSA P-256 / SHA-256 private key in the shape of concord::util::openssl_utils::AsymmetricPrivateKey
// (util/include/openssl_crypto.hpp), the counterpart of HipP256PublicKey: built from the serialised form
// "PRIVATE_KEY:secp256r1:<hex scalar>", signs to DER.  The reference signs with EVP_DigestSign and a random
// nonce; here the nonce is RFC 6979's, so a signature is reproducible: sign() runs the GPU's
// lane code (csrc/ecdsa_p256_sign.h) built for the host, signBatch() the GPU from gpuMinBatchP256Sign()
// requests up, byte for byte the same; csrc/ecdsa_der.h writes the DER form.
class HipP256PrivateKey {
 public:
  // Throws std::invalid_argument unless `serialized` is PRIVATE_KEY:secp256r1: and a hex scalar in [1, n - 1].
  explicit HipP256PrivateKey(const std::string& serialized);
  ~HipP256PrivateKey();  // unloads the key from the GPU and wipes the scalar
  HipP256PrivateKey(const HipP256PrivateKey&) = delete;
  HipP256PrivateKey& operator=(const HipP256PrivateKey&) = delete;

  std::string sign(const std::string& message) const;  // DER SEQUENCE { INTEGER r, INTEGER s }
  std::string serialize() const;                       // PRIVATE_KEY:secp256r1:<scalar>, upper-case hex as BN_bn2hex
  std::string publicKeySerialized() const;             // PUBLIC_KEY:secp256r1:04<X><Y>, as HipP256PublicKey takes it

  struct Request {
    const HipP256PrivateKey* key;
    const char* data;
    size_t dataLength;
    std::string* outSig;  // receives the DER signature
  };
  // *reqs[i].outSig = reqs[i].key->sign(reqs[i].data) for every request.  gpuMinBatchP256Sign() requests or more:
  // one cbft_ecdsa_sign_batch call per distinct key on the process's ECDSA engine (a key is loaded into it at
  // its first such batch); below that count, or for a key whose GPU call fails (counted in
  // ecdsaP256SignStats().gpu_errors), the host loop over sign().  A request with a null key or outSig is skipped.
  static void signBatch(std::vector<Request>& reqs);
  static size_t gpuMinBatchP256Sign();

 private:
  void signRaw(const char* data, size_t len, uint8_t rs[64]) const;
  uint8_t scalar_[32];  // big-endian; wiped by the destructor
  uint8_t pub_[64];     // X || Y
  mutable std::shared_ptr<EcdsaEngine> engine_;  // set once the key is loaded for signBatch
  mutable uint32_t signer_table_ = 0;
};

// Smallest secp256k1 HipECDSASigner::signBatch that goes to the GPU ($CBFT_ECDSA_SIGN_GPU_MIN
// overrides): the measured crossover of one cbft_ecdsa_sign_batch call, host arrays in to host
// arrays out, against a loop of sign() (the lane code built for the host) on one core, rounded up to
// a power of two: 16 (profiles/ecdsa_sign.json "crossover").
#define CBFT_ECDSA_SIGN_GPU_MIN_DEFAULT 16

// ECDSA / SHA-256 signing in place of concord::util::crypto::ECDSASigner (Crypto++ ECDSA<ECP,
// SHA256>::Signer, util/include/crypto_utils.hpp:71-90).  Signatures are r || s, each as long as the
// group order.  A secp256k1 key signs with RFC 6979 nonces: sign() runs the GPU's
// lane code built for the host (the same bytes, the same constant-time construction), signBatch()
// one GPU call from gpuMinBatch() requests up.  A key on any other curve the host OpenSSL knows
// (KeyExchangeManager generates secp384r1 keys) signs with OpenSSL on the host only.
class HipECDSASigner : public ISigner {
 public:
  // An EC private key, hex DER (PKCS#8 or RFC 5915) or PEM.  Throws std::invalid_argument unless it
  // parses as an EC private key on a named curve.
  HipECDSASigner(const std::string& str_priv_key, KeyFormat fmt);
  ~HipECDSASigner() override;  // wipes the private scalar
  HipECDSASigner(const HipECDSASigner&) = delete;
  HipECDSASigner& operator=(const HipECDSASigner&) = delete;

  std::string sign(const std::string& data) override;
  // reqs[i].outSig = sign(reqs[i].data) for every request.  secp256k1 and gpuMinBatch() requests or
  // more: one cbft_ecdsa_sign_batch call on the process's ECDSA engine (the key is loaded into it at
  // the first such batch); below it, on another curve, or when the GPU call fails (counted in
  // ecdsaSignStats().gpu_errors), the host loop over sign().  Throws only where sign() throws.
  void signBatch(const std::vector<SignRequest>& reqs);
  static size_t gpuMinBatch();
  uint32_t signatureLength() const override { return sig_len_; }
  std::string getPrivKey() const override { return key_str_; }
  bool gpuCapable() const { return gpu_capable_; }
  // the public key as HipECDSAVerifier takes it (X.509 SubjectPublicKeyInfo, hex DER)
  std::string getPubKeyHex() const;

 private:
  std::string key_str_;
  uint32_t sig_len_ = 0;
  bool gpu_capable_ = false;
  void* pkey_ = nullptr;  // EVP_PKEY*
  uint8_t scalar_[32];    // secp256k1: the private scalar, big-endian; wiped by the destructor
  std::shared_ptr<EcdsaEngine> engine_;  // set once the key is loaded for signBatch
  uint32_t signer_table_ = 0;
};

class EdDSASigner : public ISigner {
 public:
  // 32-byte RFC 8032 seed in hex, or a PKCS#8 PEM private key
  EdDSASigner(const std::string& str_priv_key, KeyFormat fmt);
  ~EdDSASigner() override;
  EdDSASigner(const EdDSASigner&) = delete;
  EdDSASigner& operator=(const EdDSASigner&) = delete;
  EdDSASigner(EdDSASigner&& o) noexcept;
  std::string sign(const std::string& data) override;
  // reqs[i].outSig = sign(reqs[i].data) for every request.  From gpuMinBatch() requests up: one
  // cbft_ed25519_sign_batch call on the process's Ed25519 engine (the seed is registered with it
  // at the first such batch); below it, or when the GPU call fails (counted in
  // ed25519SignStats().gpu_errors), the host loop over sign().  Throws only where sign() throws.
  void signBatch(const std::vector<SignRequest>& reqs);
  static size_t gpuMinBatch();
  uint32_t signatureLength() const override { return 64; }
  std::string getPrivKey() const override { return key_str_; }
  std::string getPubKeyHex() const;

 private:
  std::string key_str_;
  void* pkey_;  // EVP_PKEY*
  uint8_t seed_[32];                       // wiped by the destructor
  std::shared_ptr<Ed25519Engine> engine_;  // set once the seed is registered for signBatch
  uint32_t signer_table_ = 0;
};

// Smallest HipRSASigner::signBatch that goes to the GPU ($CBFT_RSA_SIGN_GPU_MIN overrides): the
// measured crossover of one cbft_rsa_sign_batch call, host arrays in to host arrays out, against
// a loop of sign() on one core, rounded up to a power of two.
#define CBFT_RSA_SIGN_GPU_MIN_DEFAULT 64

// The reference's RSASigner (sign(), signatureLength(), getPrivKey() inherited unchanged) with the
// batch form of sign().
class HipRSASigner : public concord::util::crypto::RSASigner {
 public:
  // hex DER (PKCS#8 or PKCS#1) or PEM, as RSASigner takes it
  HipRSASigner(const std::string& str_priv_key, KeyFormat fmt);
  ~HipRSASigner() override;
  HipRSASigner(const HipRSASigner&) = delete;
  HipRSASigner& operator=(const HipRSASigner&) = delete;
  // reqs[i].outSig = sign(reqs[i].data) (256 bytes for a 2,048-bit key) for every request.  From
  // gpuMinBatch() requests up: one cbft_rsa_sign_batch call on the process's RSA engine (the CRT
  // parameters are registered with it at the first such batch).  Below it, when the GPU call fails
  // (counted in rsaSignStats().gpu_errors) and for the items the device's fault check withheld:
  // sign().  A key that is not 2,048-bit two-prime with a 32-bit e never uses the GPU.
  void signBatch(const std::vector<SignRequest>& reqs);
  static size_t gpuMinBatch();
  bool gpuCapable() const { return gpu_capable_; }

 private:
  bool gpu_capable_ = false;
  uint8_t priv_[640];  // p | q | dP | dQ | qInv, big-endian; wiped by the destructor
  uint32_t e_ = 0;
  std::shared_ptr<RsaEngine> engine_;  // set once the key is registered for signBatch
  uint32_t signer_table_ = 0;
};

enum class KeyKind { Ed25519, RSA, Unknown };
// What a public-key string holds (Ed25519: raw 32 bytes or its SubjectPublicKeyInfo; RSA: an
// RSA SubjectPublicKeyInfo), without registering it anywhere.
KeyKind publicKeyKind(const std::string& str_pub_key, KeyFormat fmt);
KeyKind privateKeyKind(const std::string& str_priv_key, KeyFormat fmt);

// The verifier a key calls for: Ed25519 -> HipEdDSAVerifier, RSA -> HipRSAVerifier; throws
// std::invalid_argument otherwise.
std::shared_ptr<IVerifier> makeVerifier(const std::string& str_pub_key, KeyFormat fmt);
// Ed25519 seed -> EdDSASigner; an RSA private key -> HipRSASigner (the reference's own
// concord::util::crypto::RSASigner with signBatch added); throws std::invalid_argument otherwise.
std::unique_ptr<ISigner> makeSigner(const std::string& str_priv_key, KeyFormat fmt);

// A mixed batch: one GPU launch per algorithm; any other IVerifier runs its own verify().
void verifyBatch(const std::vector<VerifyRequest>& reqs, std::vector<bool>& out);

// Key-string helpers shared by the parsers.
std::string toHex(const uint8_t* p, size_t n);
bool fromHex(const std::string& hex, std::vector<uint8_t>& out);
bool parseEd25519PublicKey(const std::string& s, KeyFormat fmt, uint8_t out[32]);
std::string ed25519PublicKeyToPem(const uint8_t raw[32]);

// Engine instrumentation.
struct EngineStats {
  uint64_t batches;      // GPU batches run for verify() / verifyBatch()
  uint64_t items;        // signatures in them
  uint64_t gpu_errors;   // batches whose GPU call failed (their signatures verified false)
  uint32_t live_keys;    // Ed25519 key slots in use
  uint32_t table_keys;   // Ed25519 key slots on the device (live + free for reuse)
};
EngineStats ed25519EngineStats();
// Signing counters of the process (they do not need an open engine).
struct SignStats {
  uint64_t gpu_batches;  // signBatch calls signed on the GPU
  uint64_t gpu_items;    // signatures in them
  uint64_t host_items;   // signatures signBatch made with the host loop
  uint64_t gpu_errors;   // signBatch calls whose GPU path failed (signed by the host loop instead)
};
SignStats ed25519SignStats();
SignStats rsaSignStats();  // the same for HipRSASigner::signBatch
SignStats ecdsaSignStats();  // the same for HipECDSASigner::signBatch
SignStats ecdsaP256SignStats();  // the same for HipP256PrivateKey::signBatch; a GPU batch is one call for one key
// prime256v1 verification in HipECDSAVerifier::verifyBatch: GPU batches and their items, items verified on
// the host below gpuMinBatchP256(), failed GPU calls (their items come out false)
struct EcdsaP256VerifyStats {
  uint64_t gpu_batches, gpu_items, host_items, gpu_errors;
};
EcdsaP256VerifyStats ecdsaP256VerifyStats();

// Selects the GPU the engines open (default 0; $CBFT_DEVICE overrides).  Call before the first
// verifier is constructed.
void setEd25519Device(int device);

}  // namespace concord::hip
