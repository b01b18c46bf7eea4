// HipECDSAVerifier and HipECDSASigner over libcbft_hipcrypto (see hip_crypto.hpp).
//
// Reference: concord::util::crypto::ECDSAVerifier (util/src/crypto_utils.cpp:34-64,231-236):
// Crypto++ ECDSA<ECP, SHA256>, default curve secp256k1, keyed from hex DER (X509PublicKey) or PEM;
// its call site is reconfiguration_handler.cpp:332-338.  Key parsing here uses the host OpenSSL
// (d2i_PUBKEY / PEM_read_bio_PUBKEY); secp256k1 batches of gpuMinBatch() items and more run on the
// GPU, smaller ones and other curves on the host OpenSSL (the GPU path reproduces its verdicts).
// prime256v1 (secp256r1, P-256) keys are GPU-capable too: they register in a table of their own in the
// same engine and go to the GPU from gpuMinBatchP256() items up.  HipP256PublicKey is the shape of
// concord::util::openssl_utils::AsymmetricPublicKey over such a key: DER signatures, undone by
// csrc/ecdsa_der.h, then the same path.
//
// Signer: concord::util::crypto::ECDSASigner (crypto_utils.cpp:66-99), keyed from hex DER or PEM of an
// EC private key.  secp256k1 keys sign with RFC 6979 nonces: sign() with the lane code of
// csrc/ecdsa_sign.h built for the host, signBatch() on the GPU from gpuMinBatch() requests up, byte
// for byte the same; other curves sign with the host OpenSSL.
//
// HipP256PrivateKey is the shape of concord::util::openssl_utils::AsymmetricPrivateKey (util/src/
// openssl_crypto.cpp, EVPPKEYPrivateKey) over a secp256r1 scalar: RFC 6979 signatures in DER, sign() with the
// lane code of csrc/ecdsa_p256_sign.h built for the host, signBatch() on the GPU from gpuMinBatchP256Sign()
// requests up, byte for byte the same.
#include <openssl/bio.h>
#include <openssl/bn.h>
#include <openssl/core_names.h>
#include <openssl/ecdsa.h>
#include <openssl/evp.h>
#include <openssl/pem.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <stdexcept>

#include <openssl/crypto.h>

#include "../../csrc/ecdsa_der.h"        // DER -> r || s for HipP256PublicKey, r || s -> DER for HipP256PrivateKey
#include "../../csrc/ecdsa_p256_sign.h"  // the P-256 signing lane code, host build
#include "../../csrc/ecdsa_sign.h"       // the signing lane code, host build
#include "cbft_hipcrypto.h"
#include "hip_crypto.hpp"

namespace concord::hip {

namespace {

EVP_PKEY* parseEcPublicKey(const std::string& s, KeyFormat fmt) {
  if (fmt == KeyFormat::HexaDecimalStrippedFormat) {
    std::vector<uint8_t> der;
    if (!fromHex(s, der) || der.empty()) return nullptr;
    const unsigned char* p = der.data();
    return d2i_PUBKEY(nullptr, &p, (long)der.size());
  }
  BIO* bio = BIO_new_mem_buf(s.data(), (int)s.size());
  if (!bio) return nullptr;
  EVP_PKEY* k = PEM_read_bio_PUBKEY(bio, nullptr, nullptr, nullptr);
  BIO_free(bio);
  return k;
}

EVP_PKEY* parseEcPrivateKey(const std::string& s, KeyFormat fmt) {
  if (fmt == KeyFormat::HexaDecimalStrippedFormat) {
    std::vector<uint8_t> der;
    if (!fromHex(s, der) || der.empty()) return nullptr;
    const unsigned char* p = der.data();
    EVP_PKEY* k = d2i_AutoPrivateKey(nullptr, &p, (long)der.size());  // PKCS#8 or RFC 5915
    OPENSSL_cleanse(der.data(), der.size());
    return k;
  }
  BIO* bio = BIO_new_mem_buf(s.data(), (int)s.size());
  if (!bio) return nullptr;
  EVP_PKEY* k = PEM_read_bio_PrivateKey(bio, nullptr, nullptr, nullptr);
  BIO_free(bio);
  return k;
}

// G's comb table for the host build of the lane code (public data), built at the first sign()
const uint32_t* hostCombTable() {
  static std::once_flag once;
  static std::vector<uint32_t> tbl;
  std::call_once(once, [] {
    tbl.assign(ECDSAS_TABLE_WORDS, 0);
    for (int j = 0; j < ECDSAS_TABLE_LANES; j++) ecdsas_table_lane(tbl.data(), j);
  });
  return tbl.data();
}

std::atomic<uint64_t> g_p256_gpu_batches{0}, g_p256_gpu_items{0}, g_p256_host_items{0}, g_p256_gpu_errors{0};
// the same for P-256 (csrc/ecdsa_p256_sign.h)
const uint32_t* hostCombTableP256() {
  static std::once_flag once;
  static std::vector<uint32_t> tbl;
  std::call_once(once, [] {
    tbl.assign(ECDSAS_TABLE_WORDS, 0);
    for (int j = 0; j < ECDSAS_TABLE_LANES; j++) p2s_table_lane(tbl.data(), j);
  });
  return tbl.data();
}

std::atomic<uint64_t> g_p256_sign_gpu_batches{0}, g_p256_sign_gpu_items{0}, g_p256_sign_host_items{0},
    g_p256_sign_gpu_errors{0};
std::atomic<uint64_t> g_sign_gpu_batches{0}, g_sign_gpu_items{0}, g_sign_host_items{0}, g_sign_gpu_errors{0};
std::mutex g_sign_register_mu;

[[noreturn]] void fail(const char* what, int rc) {
  throw std::runtime_error(std::string(what) + ": " + cbft_strerror(rc) + " " + cbft_last_error());
}

}  // namespace

// Per-process owner of the GPU context and the device ECDSA key table (keys deduplicated, the
// table rebuilt lazily before the first batch that needs a newly registered key) -- the twin of
// RsaEngine in hip_rsa.cpp.
class EcdsaEngine {
 public:
  static std::shared_ptr<EcdsaEngine> get() {
    static std::mutex m;
    static std::weak_ptr<EcdsaEngine> inst;
    std::lock_guard<std::mutex> g(m);
    auto sp = inst.lock();
    if (!sp) {
      sp = std::shared_ptr<EcdsaEngine>(new EcdsaEngine());
      inst = sp;
    }
    return sp;
  }
  ~EcdsaEngine() {
    if (ctx_) cbft_close(ctx_);
  }

  // registration needs no GPU: the context is opened by the first batch
  // curve: CBFT_CURVE_*; each curve has its own key set and device table, indices count per curve
  uint32_t registerKey(int curve, const uint8_t pub[64]) {
    std::lock_guard<std::mutex> g(mu_);
    KeySet& ks = sets_[curve];
    std::string k(reinterpret_cast<const char*>(pub), 64);
    auto it = ks.index.find(k);
    if (it != ks.index.end()) return it->second;
    const uint32_t idx = (uint32_t)(ks.pubs.size() / 64);
    ks.pubs.insert(ks.pubs.end(), pub, pub + 64);
    ks.index.emplace(std::move(k), idx);
    return idx;
  }

  // Signer tables of HipECDSASigner::signBatch: one per signer object, loaded at its first GPU batch.
  int loadSigner(const uint8_t priv[32], uint32_t* id) {
    open();
    return cbft_ecdsa_load_signers(ctx_, priv, 1, id);
  }
  // the same on a named curve (HipP256PrivateKey::signBatch)
  int loadSignerCurve(int curve, const uint8_t priv[32], uint32_t* id) {
    open();
    return cbft_ecdsa_load_signers_curve(ctx_, curve, priv, 1, id);
  }
  void unloadSigner(uint32_t id) { (void)cbft_ecdsa_unload_signers(ctx_, id); }
  int signBatch(uint32_t id, const uint8_t* blob, const uint64_t* off, const uint32_t* len, size_t n, uint8_t* sig) {
    return cbft_ecdsa_sign_batch(ctx_, id, nullptr, blob, off, len, n, sig);
  }

  // one batch of 64-byte signatures; GPU failures become false verdicts and are counted
  // returns false when the GPU call failed
  bool verifyNoThrow(int curve, const std::vector<uint32_t>& kidx, const std::vector<uint8_t>& sig, const std::vector<uint8_t>& msg,
                     const std::vector<uint64_t>& off, const std::vector<uint32_t>& len, std::vector<uint8_t>& bitmap) {
    try {
      verify(curve, kidx, sig, msg, off, len, bitmap);
      return true;
    } catch (...) {
      if (curve == CBFT_CURVE_P256)
        g_p256_gpu_errors++;  // read by ecdsaP256VerifyStats()
      else
        gpu_errors_++;
      std::fill(bitmap.begin(), bitmap.end(), 0);
      return false;
    }
  }

 private:
  static constexpr uint32_t kNoTable = 0;  // table ids start at 1
  struct KeySet {  // one curve's registered keys and their device table
    std::vector<uint8_t> pubs;
    std::map<std::string, uint32_t> index;
    uint32_t table = kNoTable;
    uint32_t loaded = 0;
  };
  EcdsaEngine() = default;

  void open() {
    std::lock_guard<std::mutex> g(mu_);
    if (ctx_) return;
    const char* e = std::getenv("CBFT_DEVICE");
    const int rc = cbft_open(&ctx_, e ? std::atoi(e) : 0, 0);
    if (rc != CBFT_OK) {
      ctx_ = nullptr;
      fail("cbft_open", rc);
    }
  }

  void verify(int curve, const std::vector<uint32_t>& kidx, const std::vector<uint8_t>& sig, const std::vector<uint8_t>& msg,
              const std::vector<uint64_t>& off, const std::vector<uint32_t>& len, std::vector<uint8_t>& bitmap) {
    open();
    KeySet& ks = sets_[curve];
    std::shared_lock<std::shared_mutex> rd(tbl_mu_);
    while (true) {
      {
        std::lock_guard<std::mutex> g(mu_);
        if (ks.loaded == ks.pubs.size() / 64 && ks.table != kNoTable) break;
      }
      rd.unlock();
      refreshTable(curve);  // builds beside the old table; verifies keep using it meanwhile
      rd.lock();
    }
    const int rc = cbft_ecdsa_verify_batch(ctx_, ks.table, kidx.data(), sig.data(), msg.data(), off.data(), len.data(),
                                           kidx.size(), bitmap.data());
    if (rc != CBFT_OK) fail("cbft_ecdsa_verify_batch", rc);
  }

  // Rebuild the device key table for the keys registered so far without blocking verifies (as
  // RsaEngine::refreshTable): records are 1 KB each and built by one kernel launch.
  void refreshTable(int curve) {
    std::lock_guard<std::mutex> b(build_mu_);
    KeySet& ks = sets_[curve];
    std::vector<uint8_t> pubs;
    {
      std::lock_guard<std::mutex> g(mu_);
      if (ks.loaded == ks.pubs.size() / 64 && ks.table != kNoTable) return;
      pubs = ks.pubs;
    }
    uint32_t id;
    const int rc = cbft_ecdsa_load_keys_curve(ctx_, curve, pubs.data(), (uint32_t)(pubs.size() / 64), &id);
    if (rc != CBFT_OK) fail("cbft_ecdsa_load_keys_curve", rc);
    uint32_t old;
    {
      std::unique_lock<std::shared_mutex> wr(tbl_mu_);
      std::lock_guard<std::mutex> g(mu_);
      old = ks.table;
      ks.table = id;
      ks.loaded = (uint32_t)(pubs.size() / 64);
    }
    if (old != kNoTable) cbft_ecdsa_unload_keys(ctx_, old);  // readers now see table_ = id
  }

  cbft_ctx* ctx_ = nullptr;
  std::mutex mu_;             // guards ctx_ (opening) and sets_
  std::shared_mutex tbl_mu_;  // device table lifetime vs in-flight verifies
  std::mutex build_mu_;       // one table rebuild at a time
  KeySet sets_[2];            // by CBFT_CURVE_*
  std::atomic<uint64_t> gpu_errors_{0};  // failed secp256k1 GPU calls (P-256 ones: g_p256_gpu_errors)
};

HipECDSAVerifier::HipECDSAVerifier(const std::string& str_pub_key, KeyFormat fmt) : key_str_(str_pub_key) {
  EVP_PKEY* k = parseEcPublicKey(str_pub_key, fmt);
  char group[80] = {0};
  size_t glen = 0;
  BIGNUM *order = nullptr, *x = nullptr, *y = nullptr;
  bool ok = k && EVP_PKEY_get_base_id(k) == EVP_PKEY_EC &&
            EVP_PKEY_get_utf8_string_param(k, OSSL_PKEY_PARAM_GROUP_NAME, group, sizeof group, &glen) == 1 &&
            EVP_PKEY_get_bn_param(k, OSSL_PKEY_PARAM_EC_ORDER, &order) == 1;
  if (ok) sig_len_ = 2u * (uint32_t)BN_num_bytes(order);
  BN_free(order);
  const bool k1 = ok && std::strcmp(group, "secp256k1") == 0, p256 = ok && std::strcmp(group, "prime256v1") == 0;
  if (k1 || p256) {
    uint8_t pub[64];
    ok = EVP_PKEY_get_bn_param(k, OSSL_PKEY_PARAM_EC_PUB_X, &x) == 1 &&
         EVP_PKEY_get_bn_param(k, OSSL_PKEY_PARAM_EC_PUB_Y, &y) == 1 && BN_bn2binpad(x, pub, 32) == 32 &&
         BN_bn2binpad(y, pub + 32, 32) == 32;
    BN_free(x);
    BN_free(y);
    if (ok) {
      curve_ = p256 ? CBFT_CURVE_P256 : CBFT_CURVE_SECP256K1;
      engine_ = EcdsaEngine::get();
      key_index_ = engine_->registerKey(curve_, pub);
      std::memcpy(pub_, pub, 64);
      gpu_capable_ = true;
    }
  }
  if (ok) {
    pkey_ = k;  // the host path: other curves, and secp256k1 below gpuMinBatch()
  } else {
    EVP_PKEY_free(k);
  }
  if (!ok) throw std::invalid_argument("HipECDSAVerifier: not an EC public key on a named curve");
}

HipECDSAVerifier::~HipECDSAVerifier() { EVP_PKEY_free(static_cast<EVP_PKEY*>(pkey_)); }

size_t HipECDSAVerifier::gpuMinBatch() {
  static const size_t v = [] {
    const char* e = std::getenv("CBFT_ECDSA_GPU_MIN");
    const long long x = e ? std::atoll(e) : 0;
    return x > 0 ? (size_t)x : (size_t)CBFT_ECDSA_GPU_MIN_DEFAULT;
  }();
  return v;
}

size_t HipECDSAVerifier::gpuMinBatchP256() {
  static const size_t v = [] {
    const char* e = std::getenv("CBFT_ECDSA_P256_GPU_MIN");
    const long long x = e ? std::atoll(e) : 0;
    return x > 0 ? (size_t)x : (size_t)CBFT_ECDSA_P256_GPU_MIN_DEFAULT;
  }();
  return v;
}

// r || s -> DER, then EVP_DigestVerify (SHA-256) on the host
bool HipECDSAVerifier::verifyHost(const char* data, size_t len, const char* sig, size_t sig_len) const {
  if (!pkey_ || sig_len != sig_len_) return false;
  const size_t half = sig_len_ / 2;
  const unsigned char* sb = reinterpret_cast<const unsigned char*>(sig);
  BIGNUM* r = BN_bin2bn(sb, (int)half, nullptr);
  BIGNUM* s = BN_bin2bn(sb + half, (int)half, nullptr);
  ECDSA_SIG* es = ECDSA_SIG_new();
  bool ok = false;
  if (r && s && es && ECDSA_SIG_set0(es, r, s) == 1) {
    r = s = nullptr;  // owned by es
    unsigned char* der = nullptr;
    const int dl = i2d_ECDSA_SIG(es, &der);
    if (dl > 0) {
      EVP_MD_CTX* md = EVP_MD_CTX_new();
      ok = md && EVP_DigestVerifyInit(md, nullptr, EVP_sha256(), nullptr, static_cast<EVP_PKEY*>(pkey_)) == 1 &&
           EVP_DigestVerify(md, der, (size_t)dl, reinterpret_cast<const unsigned char*>(data), len) == 1;
      EVP_MD_CTX_free(md);
    }
    OPENSSL_free(der);
  }
  BN_free(r);
  BN_free(s);
  ECDSA_SIG_free(es);
  return ok;
}

bool HipECDSAVerifier::verify(const std::string& data, const std::string& sig) const {
  std::vector<VerifyRequest> r{{this, data.data(), data.size(), sig.data(), sig.size()}};
  std::vector<bool> out;
  verifyBatch(r, out);
  return out[0];
}

void HipECDSAVerifier::verifyBatch(const std::vector<VerifyRequest>& reqs, std::vector<bool>& out) {
  out.assign(reqs.size(), false);
  std::vector<size_t> pos[2];  // GPU-capable requests by CBFT_CURVE_*
  std::shared_ptr<EcdsaEngine> engine;
  for (size_t i = 0; i < reqs.size(); i++) {
    auto v = dynamic_cast<const HipECDSAVerifier*>(reqs[i].verifier);
    if (!v) continue;
    if (!v->gpu_capable_) {
      out[i] = v->verifyHost(reqs[i].data, reqs[i].dataLength, reqs[i].sig, reqs[i].sigLength);
      continue;
    }
    if (reqs[i].sigLength != CBFT_ECDSA_SIGNATURE_BYTES || reqs[i].dataLength > 0xFFFFFF00u) continue;
    engine = v->engine_;
    pos[v->curve_].push_back(i);
  }
  for (int curve = 0; curve < 2; curve++) {  // each curve's group goes to the GPU at its own minimum
    const std::vector<size_t>& ps = pos[curve];
    if (ps.empty()) continue;
    const bool p256 = curve == CBFT_CURVE_P256;
    const size_t n = ps.size();
    if (n < (p256 ? gpuMinBatchP256() : gpuMinBatch())) {  // a host loop is faster than one GPU call
      for (size_t i : ps)
        out[i] = static_cast<const HipECDSAVerifier*>(reqs[i].verifier)
                     ->verifyHost(reqs[i].data, reqs[i].dataLength, reqs[i].sig, reqs[i].sigLength);
      if (p256) g_p256_host_items += n;
      continue;
    }
    size_t blob = 0;
    for (size_t i : ps) blob += reqs[i].dataLength;
    std::vector<uint32_t> kidx(n), len(n);
    std::vector<uint64_t> off(n);
    std::vector<uint8_t> sig(n * CBFT_ECDSA_SIGNATURE_BYTES), msg(blob ? blob : 1), bitmap((n + 7) / 8);
    size_t o = 0;
    for (size_t j = 0; j < n; j++) {
      const VerifyRequest& r = reqs[ps[j]];
      kidx[j] = static_cast<const HipECDSAVerifier*>(r.verifier)->key_index_;
      std::memcpy(&sig[CBFT_ECDSA_SIGNATURE_BYTES * j], r.sig, CBFT_ECDSA_SIGNATURE_BYTES);
      off[j] = o;
      len[j] = (uint32_t)r.dataLength;
      if (r.dataLength) std::memcpy(&msg[o], r.data, r.dataLength);
      o += r.dataLength;
    }
    const bool ran = engine->verifyNoThrow(curve, kidx, sig, msg, off, len, bitmap);
    if (p256) {
      if (ran) {  // a failed call is counted where it is caught (EcdsaEngine::verifyNoThrow)
        g_p256_gpu_batches++;
        g_p256_gpu_items += n;
      }
    }
    for (size_t j = 0; j < n; j++) out[ps[j]] = (bitmap[j >> 3] >> (j & 7)) & 1;
  }
}

EcdsaP256VerifyStats ecdsaP256VerifyStats() {
  return EcdsaP256VerifyStats{g_p256_gpu_batches.load(), g_p256_gpu_items.load(), g_p256_host_items.load(), g_p256_gpu_errors.load()};
}

// ---- HipP256PublicKey ----------------------------------------------------------------------------
namespace {
const char kP256Prefix[] = "PUBLIC_KEY:secp256r1:";
}

HipP256PublicKey::HipP256PublicKey(const std::string& serialized) {
  const size_t pl = sizeof kP256Prefix - 1;
  std::vector<uint8_t> point;
  if (serialized.compare(0, pl, kP256Prefix) != 0 || !fromHex(serialized.substr(pl), point) || point.empty())
    throw std::invalid_argument("HipP256PublicKey: not PUBLIC_KEY:secp256r1:<hex point>");
  // the point in any of the forms EC_POINT_point2hex writes (uncompressed, compressed, hybrid)
  char group[] = "prime256v1";
  OSSL_PARAM params[] = {OSSL_PARAM_construct_utf8_string(OSSL_PKEY_PARAM_GROUP_NAME, group, 0),
                         OSSL_PARAM_construct_octet_string(OSSL_PKEY_PARAM_PUB_KEY, point.data(), point.size()),
                         OSSL_PARAM_construct_end()};
  EVP_PKEY_CTX* pc = EVP_PKEY_CTX_new_from_name(nullptr, "EC", nullptr);
  EVP_PKEY* k = nullptr;
  const bool ok = pc && EVP_PKEY_fromdata_init(pc) == 1 && EVP_PKEY_fromdata(pc, &k, EVP_PKEY_PUBLIC_KEY, params) == 1;
  EVP_PKEY_CTX_free(pc);
  unsigned char* der = nullptr;
  const int n = ok ? i2d_PUBKEY(k, &der) : 0;
  EVP_PKEY_free(k);
  if (n <= 0) throw std::invalid_argument("HipP256PublicKey: not a point on secp256r1");
  const std::string hex = toHex(der, (size_t)n);
  OPENSSL_free(der);
  verifier_.reset(new HipECDSAVerifier(hex, KeyFormat::HexaDecimalStrippedFormat));
}

HipP256PublicKey::~HipP256PublicKey() = default;

std::string HipP256PublicKey::serialize() const {
  // the uncompressed point in upper-case hex, as EC_POINT_point2hex writes it for this group
  static const char* d = "0123456789ABCDEF";
  std::string out = kP256Prefix;
  out += "04";
  for (int i = 0; i < 64; i++) {
    out += d[verifier_->pub_[i] >> 4];
    out += d[verifier_->pub_[i] & 15];
  }
  return out;
}

bool HipP256PublicKey::verify(const std::string& message, const std::string& der_signature) const {
  std::vector<Request> r{{this, message.data(), message.size(), der_signature.data(), der_signature.size()}};
  std::vector<bool> out;
  verifyBatch(r, out);
  return out[0];
}

void HipP256PublicKey::verifyBatch(const std::vector<Request>& reqs, std::vector<bool>& out) {
  out.assign(reqs.size(), false);
  std::vector<uint8_t> rs(reqs.size() * 64);
  std::vector<VerifyRequest> vr;
  std::vector<size_t> pos;
  for (size_t i = 0; i < reqs.size(); i++) {
    if (!reqs[i].key) continue;
    if (!ecdsa_der_to_rs(reinterpret_cast<const uint8_t*>(reqs[i].sig), reqs[i].sigLength, 32, &rs[64 * i])) continue;
    vr.push_back({reqs[i].key->verifier_.get(), reqs[i].data, reqs[i].dataLength,
                  reinterpret_cast<const char*>(&rs[64 * i]), 64});
    pos.push_back(i);
  }
  std::vector<bool> got;
  HipECDSAVerifier::verifyBatch(vr, got);
  for (size_t j = 0; j < pos.size(); j++) out[pos[j]] = got[j];
}

// ---- HipP256PrivateKey ---------------------------------------------------------------------------
namespace {
const char kP256PrivPrefix[] = "PRIVATE_KEY:secp256r1:";
const char kHexUpper[] = "0123456789ABCDEF";
}  // namespace

HipP256PrivateKey::HipP256PrivateKey(const std::string& serialized) {
  std::memset(scalar_, 0, sizeof scalar_);
  std::memset(pub_, 0, sizeof pub_);
  const size_t a = serialized.find(':'), b = a == std::string::npos ? a : serialized.find(':', a + 1);
  if (b == std::string::npos || serialized.compare(0, a, "PRIVATE_KEY") != 0)
    throw std::invalid_argument("HipP256PrivateKey: input is not labeled as a private key");
  if (serialized.compare(a + 1, b - a - 1, "secp256r1") != 0)
    throw std::invalid_argument("HipP256PrivateKey: scheme is not secp256r1");
  // the scalar as BN_hex2bn reads it: hex digits of either case, any number of leading zeros
  size_t i = b + 1;
  const size_t end = serialized.size();
  bool ok = i < end;
  while (i < end && serialized[i] == '0') i++;
  ok = ok && end - i <= 64;
  uint8_t nib[64] = {0};
  for (size_t j = i; ok && j < end; j++) {
    const char c = serialized[j];
    const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
    ok = v >= 0;
    if (ok) nib[64 - (end - j)] = (uint8_t)v;
  }
  if (!ok) {
    OPENSSL_cleanse(nib, sizeof nib);
    throw std::invalid_argument("HipP256PrivateKey: key data is not a hexadecimal scalar of at most 256 bits");
  }
  for (int j = 0; j < 32; j++) scalar_[j] = (uint8_t)((nib[2 * j] << 4) | nib[2 * j + 1]);
  OPENSSL_cleanse(nib, sizeof nib);
  // range check and public key by the lane code: 0 or >= n gives a record with its validity clear
  uint32_t rec[ECDSAS_WORDS];
  p2s_signer_lane(rec, scalar_, hostCombTableP256());
  const bool usable = rec[ECDSAS_OK] != 0;
  k1_to_be(pub_, rec + 8);
  k1_to_be(pub_ + 32, rec + 16);
  OPENSSL_cleanse(rec, sizeof rec);
  if (!usable) {
    OPENSSL_cleanse(scalar_, sizeof scalar_);
    throw std::invalid_argument("HipP256PrivateKey: the scalar is 0 or not below the group order");
  }
}

HipP256PrivateKey::~HipP256PrivateKey() {
  if (engine_) engine_->unloadSigner(signer_table_);
  OPENSSL_cleanse(scalar_, sizeof scalar_);
}

size_t HipP256PrivateKey::gpuMinBatchP256Sign() {
  static const size_t v = [] {
    const char* e = std::getenv("CBFT_ECDSA_P256_SIGN_GPU_MIN");
    const long long x = e ? std::atoll(e) : 0;
    return x > 0 ? (size_t)x : (size_t)CBFT_ECDSA_P256_SIGN_GPU_MIN_DEFAULT;
  }();
  return v;
}

std::string HipP256PrivateKey::serialize() const {
  std::string out = kP256PrivPrefix;
  int i = 0;
  while (i < 31 && scalar_[i] == 0) i++;  // BN_bn2hex: whole bytes, no leading zero byte
  for (; i < 32; i++) {
    out += kHexUpper[scalar_[i] >> 4];
    out += kHexUpper[scalar_[i] & 15];
  }
  return out;
}

std::string HipP256PrivateKey::publicKeySerialized() const {
  std::string out = kP256Prefix;
  out += "04";
  for (int i = 0; i < 64; i++) {
    out += kHexUpper[pub_[i] >> 4];
    out += kHexUpper[pub_[i] & 15];
  }
  return out;
}

// r || s by the lane code of the GPU kernels, built for the host: the same bytes, the same construction
void HipP256PrivateKey::signRaw(const char* data, size_t len, uint8_t rs[64]) const {
  if (len > 0xFFFFFFFFull) throw std::runtime_error("HipP256PrivateKey: message too long");
  uint32_t x[8], h1[8], sig[16];
  k1_from_be(x, scalar_);
  ecdsa_sha256(h1, reinterpret_cast<const uint8_t*>(data), (uint32_t)len);
  p2s_sign_lane(sig, x, h1, hostCombTableP256());
  std::memcpy(rs, sig, 64);
  OPENSSL_cleanse(x, sizeof x);
}

namespace {
std::string derOf(const uint8_t rs[64]) {
  uint8_t der[ECDSA_DER_MAX_BYTES(32)];
  size_t n = 0;
  if (!ecdsa_rs_to_der(rs, 32, der, &n)) throw std::runtime_error("HipP256PrivateKey: DER encoding failed");
  return std::string(reinterpret_cast<const char*>(der), n);
}
}  // namespace

std::string HipP256PrivateKey::sign(const std::string& message) const {
  uint8_t rs[64];
  signRaw(message.data(), message.size(), rs);
  return derOf(rs);
}

void HipP256PrivateKey::signBatch(std::vector<Request>& reqs) {
  std::vector<size_t> live;
  for (size_t i = 0; i < reqs.size(); i++)
    if (reqs[i].key && reqs[i].outSig) live.push_back(i);
  if (live.empty()) return;
  std::vector<bool> done(reqs.size(), false);
  if (live.size() >= gpuMinBatchP256Sign()) {
    std::map<const HipP256PrivateKey*, std::vector<size_t>> byKey;  // one signer table, one call, per key
    for (size_t i : live) byKey[reqs[i].key].push_back(i);
    for (auto& kv : byKey) {
      const HipP256PrivateKey* key = kv.first;
      const std::vector<size_t>& ps = kv.second;
      const size_t n = ps.size();
      try {
        {
          std::lock_guard<std::mutex> g(g_sign_register_mu);
          if (!key->engine_) {
            auto engine = EcdsaEngine::get();
            uint32_t id = 0;
            const int rc = engine->loadSignerCurve(CBFT_CURVE_P256, key->scalar_, &id);  // throws when the engine cannot be opened
            if (rc != CBFT_OK) throw std::runtime_error("cbft_ecdsa_load_signers_curve");
            key->engine_ = std::move(engine);
            key->signer_table_ = id;
          }
        }
        size_t blob = 0;
        bool fits = true;
        for (size_t i : ps) {
          fits = fits && reqs[i].dataLength <= 0xFFFFFF00u;
          blob += reqs[i].dataLength;
        }
        if (!fits) throw std::runtime_error("message too long for the GPU signer");
        std::vector<uint8_t> msg(blob ? blob : 1), sig(n * 64);
        std::vector<uint64_t> off(n);
        std::vector<uint32_t> len(n);
        size_t o = 0;
        for (size_t j = 0; j < n; j++) {
          const Request& r = reqs[ps[j]];
          off[j] = o;
          len[j] = (uint32_t)r.dataLength;
          if (r.dataLength) std::memcpy(&msg[o], r.data, r.dataLength);
          o += r.dataLength;
        }
        const int rc = key->engine_->signBatch(key->signer_table_, msg.data(), off.data(), len.data(), n, sig.data());
        if (rc != CBFT_OK) throw std::runtime_error("cbft_ecdsa_sign_batch");
        for (size_t j = 0; j < n; j++) {
          *reqs[ps[j]].outSig = derOf(&sig[64 * j]);
          done[ps[j]] = true;
        }
        g_p256_sign_gpu_batches++;
        g_p256_sign_gpu_items += n;
      } catch (...) {
        g_p256_sign_gpu_errors++;
      }
    }
  }
  uint64_t host = 0;
  for (size_t i : live) {
    if (done[i]) continue;
    uint8_t rs[64];
    reqs[i].key->signRaw(reqs[i].data, reqs[i].dataLength, rs);
    *reqs[i].outSig = derOf(rs);
    host++;
  }
  g_p256_sign_host_items += host;
}

SignStats ecdsaP256SignStats() {
  return SignStats{g_p256_sign_gpu_batches.load(), g_p256_sign_gpu_items.load(), g_p256_sign_host_items.load(),
                   g_p256_sign_gpu_errors.load()};
}

// ---- HipECDSASigner ------------------------------------------------------------------------------
HipECDSASigner::HipECDSASigner(const std::string& str_priv_key, KeyFormat fmt) : key_str_(str_priv_key) {
  std::memset(scalar_, 0, sizeof scalar_);
  EVP_PKEY* k = parseEcPrivateKey(str_priv_key, fmt);
  char group[80] = {0};
  size_t glen = 0;
  BIGNUM *order = nullptr, *d = nullptr;
  bool ok = k && EVP_PKEY_get_base_id(k) == EVP_PKEY_EC &&
            EVP_PKEY_get_utf8_string_param(k, OSSL_PKEY_PARAM_GROUP_NAME, group, sizeof group, &glen) == 1 &&
            EVP_PKEY_get_bn_param(k, OSSL_PKEY_PARAM_EC_ORDER, &order) == 1 &&
            EVP_PKEY_get_bn_param(k, OSSL_PKEY_PARAM_PRIV_KEY, &d) == 1;
  if (ok) sig_len_ = 2u * (uint32_t)BN_num_bytes(order);
  if (ok && std::strcmp(group, "secp256k1") == 0) {
    ok = BN_bn2binpad(d, scalar_, 32) == 32;
    gpu_capable_ = ok;
  }
  BN_free(order);
  BN_clear_free(d);
  if (!ok) {
    EVP_PKEY_free(k);
    OPENSSL_cleanse(scalar_, sizeof scalar_);
    throw std::invalid_argument("HipECDSASigner: not an EC private key on a named curve");
  }
  pkey_ = k;
}

HipECDSASigner::~HipECDSASigner() {
  if (engine_) engine_->unloadSigner(signer_table_);
  OPENSSL_cleanse(scalar_, sizeof scalar_);
  EVP_PKEY_free(static_cast<EVP_PKEY*>(pkey_));
}

size_t HipECDSASigner::gpuMinBatch() {
  static const size_t v = [] {
    const char* e = std::getenv("CBFT_ECDSA_SIGN_GPU_MIN");
    const long long x = e ? std::atoll(e) : 0;
    return x > 0 ? (size_t)x : (size_t)CBFT_ECDSA_SIGN_GPU_MIN_DEFAULT;
  }();
  return v;
}

std::string HipECDSASigner::getPubKeyHex() const {
  unsigned char* der = nullptr;
  const int n = i2d_PUBKEY(static_cast<EVP_PKEY*>(pkey_), &der);
  if (n <= 0) throw std::runtime_error("HipECDSASigner: i2d_PUBKEY");
  std::string hex = toHex(der, (size_t)n);
  OPENSSL_free(der);
  return hex;
}

std::string HipECDSASigner::sign(const std::string& data) {
  std::string out(sig_len_, '\0');
  if (gpu_capable_) {
    if (data.size() > 0xFFFFFFFFull) throw std::runtime_error("HipECDSASigner: message too long");
    // the lane code of the GPU kernels, built for the host: the same bytes, the same construction
    uint32_t rec[ECDSAS_WORDS], h1[8], sig[16];
    ecdsas_signer_lane(rec, scalar_, hostCombTable());
    if (!rec[ECDSAS_OK]) throw std::runtime_error("HipECDSASigner: private scalar out of range");
    ecdsa_sha256(h1, reinterpret_cast<const uint8_t*>(data.data()), (uint32_t)data.size());
    ecdsas_sign_lane(sig, rec, h1, hostCombTable());
    std::memcpy(&out[0], sig, 64);
    OPENSSL_cleanse(rec, sizeof rec);
    return out;
  }
  // another curve: EVP_DigestSign (SHA-256) on the host, DER -> r || s
  EVP_MD_CTX* md = EVP_MD_CTX_new();
  size_t dl = 0;
  std::vector<unsigned char> der;
  const unsigned char* m = reinterpret_cast<const unsigned char*>(data.data());
  bool ok = md && EVP_DigestSignInit(md, nullptr, EVP_sha256(), nullptr, static_cast<EVP_PKEY*>(pkey_)) == 1 &&
            EVP_DigestSign(md, nullptr, &dl, m, data.size()) == 1;
  if (ok) {
    der.resize(dl);
    ok = EVP_DigestSign(md, der.data(), &dl, m, data.size()) == 1;
  }
  EVP_MD_CTX_free(md);
  ECDSA_SIG* es = nullptr;
  if (ok) {
    const unsigned char* p = der.data();
    es = d2i_ECDSA_SIG(nullptr, &p, (long)dl);
  }
  const int half = (int)(sig_len_ / 2);
  ok = es && BN_bn2binpad(ECDSA_SIG_get0_r(es), reinterpret_cast<unsigned char*>(&out[0]), half) == half &&
       BN_bn2binpad(ECDSA_SIG_get0_s(es), reinterpret_cast<unsigned char*>(&out[half]), half) == half;
  ECDSA_SIG_free(es);
  if (!ok) throw std::runtime_error("HipECDSASigner: EVP_DigestSign failed");
  return out;
}

void HipECDSASigner::signBatch(const std::vector<SignRequest>& reqs) {
  const size_t n = reqs.size();
  if (n == 0) return;
  bool onGpu = false;
  if (gpu_capable_ && n >= gpuMinBatch()) {
    try {
      {
        std::lock_guard<std::mutex> g(g_sign_register_mu);
        if (!engine_) {
          auto engine = EcdsaEngine::get();
          uint32_t id = 0;
          const int rc = engine->loadSigner(scalar_, &id);  // throws when the engine cannot be opened
          if (rc != CBFT_OK) throw std::runtime_error("cbft_ecdsa_load_signers");
          engine_ = std::move(engine);
          signer_table_ = id;
        }
      }
      size_t blob = 0;
      bool fits = true;
      for (const SignRequest& r : reqs) {
        fits = fits && r.dataLength <= 0xFFFFFF00u;
        blob += r.dataLength;
      }
      if (!fits) throw std::runtime_error("message too long for the GPU signer");
      std::vector<uint8_t> msg(blob ? blob : 1), sig(n * 64);
      std::vector<uint64_t> off(n);
      std::vector<uint32_t> len(n);
      size_t o = 0;
      for (size_t i = 0; i < n; i++) {
        off[i] = o;
        len[i] = (uint32_t)reqs[i].dataLength;
        if (reqs[i].dataLength) std::memcpy(&msg[o], reqs[i].data, reqs[i].dataLength);
        o += reqs[i].dataLength;
      }
      const int rc = engine_->signBatch(signer_table_, msg.data(), off.data(), len.data(), n, sig.data());
      if (rc != CBFT_OK) throw std::runtime_error("cbft_ecdsa_sign_batch");
      for (size_t i = 0; i < n; i++) std::memcpy(reqs[i].outSig, &sig[64 * i], 64);
      g_sign_gpu_batches++;
      g_sign_gpu_items += n;
      onGpu = true;
    } catch (...) {
      g_sign_gpu_errors++;
    }
  }
  if (onGpu) return;
  for (const SignRequest& r : reqs) {
    const std::string s = sign(std::string(r.data, r.dataLength));
    std::memcpy(r.outSig, s.data(), s.size());
  }
  g_sign_host_items += n;
}

SignStats ecdsaSignStats() {
  return SignStats{g_sign_gpu_batches.load(), g_sign_gpu_items.load(), g_sign_host_items.load(), g_sign_gpu_errors.load()};
}

}  // namespace concord::hip
