// Host-side test of the P-256 half of the plugin layer (hip_crypto.hpp): concord::hip::HipECDSAVerifier
// on a prime256v1 key from hex DER and from PEM, and concord::hip::HipP256PublicKey from the serialised
// form PUBLIC_KEY:secp256r1:<hex point> with DER signatures, both against the host OpenSSL.  `--no-gpu`
// runs the whole test under the GPU minimum (the minima are set far above the batch sizes, so every item takes
// the host path and nothing needs a GPU); without it $CBFT_ECDSA_P256_GPU_MIN and $CBFT_ECDSA_GPU_MIN are set to 1
// so that every item, lone ones included, runs on the GPU.
#include <openssl/bio.h>
#include <openssl/ec.h>
#include <openssl/ecdsa.h>
#include <openssl/evp.h>
#include <openssl/pem.h>
#include <openssl/x509.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "hip_crypto.hpp"

using namespace concord::hip;

static int g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      g_fail++;                                                   \
    }                                                             \
  } while (0)

struct Key {
  EVP_PKEY* pkey;
  std::string hex, pem, serialized, compressed;
};

// the uncompressed point 04 || X || Y in upper-case hex, as EC_POINT_point2hex writes it
static std::string pointHex(EVP_PKEY* k) {
  unsigned char buf[80];
  size_t n = 0;
  if (EVP_PKEY_get_octet_string_param(k, "encoded-pub-key", buf, sizeof buf, &n) != 1 || n != 65 || buf[0] != 4)
    throw std::runtime_error("encoded-pub-key");
  static const char* d = "0123456789ABCDEF";
  std::string out;
  for (size_t i = 0; i < n; i++) {
    out += d[buf[i] >> 4];
    out += d[buf[i] & 15];
  }
  return out;
}

static Key makeKey(const char* curve) {
  Key k;
  k.pkey = EVP_EC_gen(curve);
  if (!k.pkey) throw std::runtime_error("EVP_EC_gen");
  unsigned char* der = nullptr;
  const int n = i2d_PUBKEY(k.pkey, &der);
  if (n <= 0) throw std::runtime_error("i2d_PUBKEY");
  k.hex = toHex(der, (size_t)n);
  OPENSSL_free(der);
  BIO* bio = BIO_new(BIO_s_mem());
  PEM_write_bio_PUBKEY(bio, k.pkey);
  char* p = nullptr;
  const long pl = BIO_get_mem_data(bio, &p);
  k.pem.assign(p, (size_t)pl);
  BIO_free(bio);
  if (std::strcmp(curve, "prime256v1") == 0) {
    const std::string pt = pointHex(k.pkey);
    const int last = pt.back() <= '9' ? pt.back() - '0' : pt.back() - 'A' + 10;
    k.serialized = "PUBLIC_KEY:secp256r1:" + pt;
    k.compressed = std::string("PUBLIC_KEY:secp256r1:") + (last & 1 ? "03" : "02") + pt.substr(2, 64);
  }
  return k;
}

// DER signature over SHA-256 by the host OpenSSL
static std::string signDer(EVP_PKEY* k, const std::string& msg) {
  EVP_MD_CTX* md = EVP_MD_CTX_new();
  size_t dl = 0;
  if (EVP_DigestSignInit(md, nullptr, EVP_sha256(), nullptr, k) != 1 ||
      EVP_DigestSign(md, nullptr, &dl, (const unsigned char*)msg.data(), msg.size()) != 1)
    throw std::runtime_error("EVP_DigestSign");
  std::string der(dl, '\0');
  if (EVP_DigestSign(md, (unsigned char*)&der[0], &dl, (const unsigned char*)msg.data(), msg.size()) != 1)
    throw std::runtime_error("EVP_DigestSign");
  EVP_MD_CTX_free(md);
  der.resize(dl);
  return der;
}

static std::string derToP1363(const std::string& der, size_t half) {
  const unsigned char* p = (const unsigned char*)der.data();
  ECDSA_SIG* es = d2i_ECDSA_SIG(nullptr, &p, (long)der.size());
  if (!es) throw std::runtime_error("d2i_ECDSA_SIG");
  std::string out(2 * half, '\0');
  BN_bn2binpad(ECDSA_SIG_get0_r(es), (unsigned char*)&out[0], (int)half);
  BN_bn2binpad(ECDSA_SIG_get0_s(es), (unsigned char*)&out[half], (int)half);
  ECDSA_SIG_free(es);
  return out;
}

// the host OpenSSL's verdict on a DER signature (what the reference's AsymmetricPublicKey::verify returns)
static bool opensslVerifyDer(EVP_PKEY* k, const std::string& msg, const std::string& der) {
  EVP_MD_CTX* md = EVP_MD_CTX_new();
  const bool ok = EVP_DigestVerifyInit(md, nullptr, EVP_sha256(), nullptr, k) == 1 &&
                  EVP_DigestVerify(md, (const unsigned char*)der.data(), der.size(), (const unsigned char*)msg.data(),
                                   msg.size()) == 1;
  EVP_MD_CTX_free(md);
  return ok;
}

// the host OpenSSL's verdict on r || s
static bool opensslVerify(EVP_PKEY* k, const std::string& msg, const std::string& sig) {
  const size_t half = sig.size() / 2;
  ECDSA_SIG* es = ECDSA_SIG_new();
  ECDSA_SIG_set0(es, BN_bin2bn((const unsigned char*)sig.data(), (int)half, nullptr),
                 BN_bin2bn((const unsigned char*)sig.data() + half, (int)half, nullptr));
  unsigned char* der = nullptr;
  const int dl = i2d_ECDSA_SIG(es, &der);
  ECDSA_SIG_free(es);
  const bool ok = dl > 0 && opensslVerifyDer(k, msg, std::string((const char*)der, (size_t)dl));
  OPENSSL_free(der);
  return ok;
}

template <class F>
static bool throwsInvalid(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  } catch (...) {
  }
  return false;
}

static void checks(bool on_gpu) {
  std::vector<Key> keys;
  std::vector<std::unique_ptr<HipECDSAVerifier>> ver;
  std::vector<std::unique_ptr<HipP256PublicKey>> pk;
  for (int i = 0; i < 4; i++) {
    keys.push_back(makeKey("prime256v1"));
    ver.emplace_back(new HipECDSAVerifier(i & 1 ? keys[i].pem : keys[i].hex,
                                          i & 1 ? KeyFormat::PemFormat : KeyFormat::HexaDecimalStrippedFormat));
    pk.emplace_back(new HipP256PublicKey(i & 1 ? keys[i].compressed : keys[i].serialized));
    CHECK(ver.back()->gpuCapable() && ver.back()->curve() == 1 && ver.back()->signatureLength() == 64);
    CHECK(pk.back()->serialize() == keys[i].serialized);  // the uncompressed form, whichever came in
    CHECK(pk.back()->verifier().engineKeyIndex() == ver.back()->engineKeyIndex());  // the same key registers once
  }
  Key k1 = makeKey("secp256k1"), k384 = makeKey("secp384r1");
  HipECDSAVerifier v1(k1.hex, KeyFormat::HexaDecimalStrippedFormat), v384(k384.hex, KeyFormat::HexaDecimalStrippedFormat);
  CHECK(v1.gpuCapable() && v1.curve() == 0 && !v384.gpuCapable());

  CHECK(throwsInvalid([] { HipP256PublicKey k("PUBLIC_KEY:secp256r1:"); }));
  CHECK(throwsInvalid([] { HipP256PublicKey k("PUBLIC_KEY:secp256r1:zz"); }));
  CHECK(throwsInvalid([&] { HipP256PublicKey k("PUBLIC_KEY:secp384r1:" + keys[0].serialized.substr(21)); }));
  CHECK(throwsInvalid([&] { HipP256PublicKey k(keys[0].serialized.substr(0, keys[0].serialized.size() - 2)); }));
  {
    std::string off = keys[0].serialized;  // a point off the curve
    off[off.size() - 1] = off[off.size() - 1] == '0' ? '1' : '0';
    CHECK(throwsInvalid([&] { HipP256PublicKey k(off); }));
  }

  // one mixed batch through HipECDSAVerifier::verifyBatch: prime256v1, secp256k1 and secp384r1 items
  const size_t n = 150;
  std::vector<std::string> msgs(n), sigs(n), ders(n);
  std::vector<bool> want(n);
  std::vector<VerifyRequest> reqs;
  for (size_t i = 0; i < n; i++) {
    msgs[i] = std::string(i % 130, (char)('a' + i % 26)) + std::to_string(i);
    const HipECDSAVerifier* who;
    if (i % 17 == 5) {
      who = &v384;
      sigs[i] = derToP1363(signDer(k384.pkey, msgs[i]), 48);
      if (i % 2) sigs[i][7] ^= 1;
      want[i] = opensslVerify(k384.pkey, msgs[i], sigs[i]);
    } else if (i % 5 == 2) {
      who = &v1;
      sigs[i] = derToP1363(signDer(k1.pkey, msgs[i]), 32);
      if (i % 3 == 0) sigs[i][40] ^= 2;
      want[i] = opensslVerify(k1.pkey, msgs[i], sigs[i]);
    } else {
      const size_t ki = i % keys.size();
      ders[i] = signDer(keys[ki].pkey, msgs[i]);
      sigs[i] = derToP1363(ders[i], 32);
      if (i % 7 == 3) sigs[i][(i * 5) % 64] ^= (char)(1 << (i % 8));
      if (i % 11 == 4) msgs[i] += "!";
      const size_t vk = i % 13 == 6 ? (ki + 1) % keys.size() : ki;  // verified under another key
      who = ver[vk].get();
      want[i] = opensslVerify(keys[vk].pkey, msgs[i], sigs[i]);
    }
    reqs.push_back({who, msgs[i].data(), msgs[i].size(), sigs[i].data(), sigs[i].size()});
  }
  size_t accepted = 0;
  for (bool w : want) accepted += w;
  CHECK(accepted > n / 2 && accepted < n);
  const EcdsaP256VerifyStats before = ecdsaP256VerifyStats();
  std::vector<bool> out;
  HipECDSAVerifier::verifyBatch(reqs, out);
  CHECK(out.size() == n);
  for (size_t i = 0; i < n; i++) CHECK(out[i] == want[i]);
  const EcdsaP256VerifyStats after = ecdsaP256VerifyStats();
  size_t np256 = 0;
  for (size_t i = 0; i < n; i++) np256 += !(i % 17 == 5) && !(i % 5 == 2);
  if (on_gpu) {
    CHECK(after.gpu_batches == before.gpu_batches + 1 && after.gpu_items == before.gpu_items + np256);
    CHECK(after.host_items == before.host_items && after.gpu_errors == before.gpu_errors);
  } else {
    CHECK(after.host_items == before.host_items + np256 && after.gpu_batches == before.gpu_batches);
  }
  for (size_t i = 0; i < 30; i++)
    CHECK(static_cast<const HipECDSAVerifier*>(reqs[i].verifier)->verify(msgs[i], sigs[i]) == want[i]);
  // wrong-length signatures are false, never an exception
  CHECK(!ver[0]->verify("x", sigs[0].substr(0, 63)) && !ver[0]->verify("x", "") && !ver[0]->verify("x", sigs[5]));

  // HipP256PublicKey: DER signatures, canonical and not, lone and in a batch, against EVP_DigestVerify
  std::vector<std::string> dm, dd;
  std::vector<size_t> dk;
  for (size_t i = 0; i < 60; i++) {
    const size_t ki = i % keys.size();
    std::string m = "der " + std::to_string(i) + std::string(i, '.');
    std::string der = signDer(keys[ki].pkey, m);
    switch (i % 10) {
      case 1: der += '\0'; break;                                        // a trailing byte
      case 2: der[der.size() - 1] ^= 1; break;                           // s damaged
      case 3: m += "!"; break;                                           // another message
      case 4: der = der.substr(0, der.size() - 1); break;                // cut short
      case 5: der = std::string("\x30\x81", 2) + der.substr(1); break;   // long-form length where the short one fits
      case 6: der.clear(); break;
      default: break;
    }
    dm.push_back(m), dd.push_back(der), dk.push_back(i % 10 == 7 ? (ki + 1) % keys.size() : ki);
  }
  std::vector<HipP256PublicKey::Request> dr;
  for (size_t i = 0; i < dm.size(); i++) dr.push_back({pk[dk[i]].get(), dm[i].data(), dm[i].size(), dd[i].data(), dd[i].size()});
  HipP256PublicKey::verifyBatch(dr, out);
  CHECK(out.size() == dm.size());
  size_t dacc = 0;
  for (size_t i = 0; i < dm.size(); i++) {
    const bool w = opensslVerifyDer(keys[dk[i]].pkey, dm[i], dd[i]);
    dacc += w;
    CHECK(out[i] == w);
    CHECK(pk[dk[i]]->verify(dm[i], dd[i]) == w);
    CHECK((i % 10 >= 1 && i % 10 <= 7) ? !w : w);
  }
  CHECK(dacc == 18);

  for (Key& k : keys) EVP_PKEY_free(k.pkey);
  EVP_PKEY_free(k1.pkey);
  EVP_PKEY_free(k384.pkey);
}

int main(int argc, char** argv) {
  const bool no_gpu = argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0;
  if (no_gpu) {  // everything under the minimum, whatever the environment says
    setenv("CBFT_ECDSA_P256_GPU_MIN", "1000000", 1);
    setenv("CBFT_ECDSA_GPU_MIN", "1000000", 1);
  } else {  // read once, at the first verify
    setenv("CBFT_ECDSA_P256_GPU_MIN", "1", 1);
    setenv("CBFT_ECDSA_GPU_MIN", "1", 1);
  }
  try {
    checks(!no_gpu);
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 2;
  }
  if (g_fail) {
    std::printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf(no_gpu ? "all checks passed under the GPU minimum\n" : "all checks passed\n");
  return 0;
}
