// Host-side test of concord::hip::HipP256PrivateKey (hip_crypto.hpp): the private half of the P-256 plugin
// layer, from the serialised form PRIVATE_KEY:secp256r1:<hex scalar>, signing to DER.  Signatures are checked
// by the host OpenSSL (EVP_DigestVerify) and by HipP256PublicKey; signBatch() must give the bytes of the sign()
// loop.  `--no-gpu` runs the whole test under the GPU minimum (the minimum is set far above the batch sizes, so
// every item takes the host path and nothing needs a GPU); without it $CBFT_ECDSA_P256_SIGN_GPU_MIN is 1, so that
// every batch, a lone request included, is signed on the GPU.
#include <openssl/bn.h>
#include <openssl/core_names.h>
#include <openssl/ec.h>
#include <openssl/evp.h>
#include <openssl/param_build.h>

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

static const char kN[] = "FFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551";
static const char kNm1[] = "FFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632550";
static const char kNp1[] = "FFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632552";
// RFC 6979 A.2.5
static const char kRfcX[] = "C9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721";
static const char kRfcPub[] =
    "PUBLIC_KEY:secp256r1:0460FED4BA255A9D31C961EB74C6356D68C049B8923B61FA6CE669622E60F29FB6"
    "7903FE1008B8BC99A41AE9E95628BC64F2F1B20C2D7E9F5177A3C294D4462299";

// the host OpenSSL's public key for the point in `serialized` (PUBLIC_KEY:secp256r1:04..)
static EVP_PKEY* opensslKey(const std::string& serialized) {
  std::vector<uint8_t> pt;
  if (!fromHex(serialized.substr(21), pt)) throw std::runtime_error("fromHex");
  char group[] = "prime256v1";
  OSSL_PARAM params[] = {OSSL_PARAM_construct_utf8_string(OSSL_PKEY_PARAM_GROUP_NAME, group, 0),
                         OSSL_PARAM_construct_octet_string(OSSL_PKEY_PARAM_PUB_KEY, pt.data(), pt.size()),
                         OSSL_PARAM_construct_end()};
  EVP_PKEY_CTX* pc = EVP_PKEY_CTX_new_from_name(nullptr, "EC", nullptr);
  EVP_PKEY* k = nullptr;
  if (!pc || EVP_PKEY_fromdata_init(pc) != 1 || EVP_PKEY_fromdata(pc, &k, EVP_PKEY_PUBLIC_KEY, params) != 1)
    throw std::runtime_error("EVP_PKEY_fromdata");
  EVP_PKEY_CTX_free(pc);
  return k;
}

// what the reference's AsymmetricPublicKey::verify returns
static bool opensslVerifyDer(EVP_PKEY* k, const std::string& msg, const std::string& der) {
  EVP_MD_CTX* md = EVP_MD_CTX_new();
  const bool ok = EVP_DigestVerifyInit(md, nullptr, EVP_sha256(), nullptr, k) == 1 &&
                  EVP_DigestVerify(md, (const unsigned char*)der.data(), der.size(), (const unsigned char*)msg.data(),
                                   msg.size()) == 1;
  EVP_MD_CTX_free(md);
  return ok;
}

static std::string hexOf(const std::string& s) { return toHex(reinterpret_cast<const uint8_t*>(s.data()), s.size()); }

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

static std::string message(size_t i) { return std::string(i % 130, (char)('a' + i % 26)) + std::to_string(i); }

static void checks(bool on_gpu) {
  const std::string P = "PRIVATE_KEY:secp256r1:";
  // constructor refusals: label, scheme, non-hex, empty, 0, n, n + 1, more than 256 bits
  CHECK(throwsInvalid([&] { HipP256PrivateKey k(std::string("PUBLIC_KEY:secp256r1:") + kRfcX); }));
  CHECK(throwsInvalid([&] { HipP256PrivateKey k(std::string("PRIVATE_KEY:secp384r1:") + kRfcX); }));
  CHECK(throwsInvalid([&] { HipP256PrivateKey k(std::string("PRIVATE_KEY:") + kRfcX); }));
  CHECK(throwsInvalid([&] { HipP256PrivateKey k{std::string(kRfcX)}; }));
  CHECK(throwsInvalid([&] { HipP256PrivateKey k(P + "C9AFA9D8zz"); }));
  CHECK(throwsInvalid([&] { HipP256PrivateKey k(P + "0x12"); }));
  CHECK(throwsInvalid([&] { HipP256PrivateKey k(P); }));
  CHECK(throwsInvalid([&] { HipP256PrivateKey k(P + "0"); }));
  CHECK(throwsInvalid([&] { HipP256PrivateKey k(P + std::string(64, '0')); }));
  CHECK(throwsInvalid([&] { HipP256PrivateKey k(P + kN); }));
  CHECK(throwsInvalid([&] { HipP256PrivateKey k(P + kNp1); }));
  CHECK(throwsInvalid([&] { HipP256PrivateKey k(P + std::string(64, 'F')); }));
  CHECK(throwsInvalid([&] { HipP256PrivateKey k(P + "1" + std::string(64, '0')); }));

  // serialize(): upper-case whole bytes without leading zero bytes (BN_bn2hex), whatever came in
  {
    HipP256PrivateKey one(P + "1"), lower(P + "00c9afa9d845ba75166b5c215767b1d6934e50c3db36e89b127b8a622b120f6721");
    HipP256PrivateKey nm1(P + kNm1), odd(P + "abc");
    CHECK(one.serialize() == P + "01");
    CHECK(lower.serialize() == P + kRfcX);
    CHECK(nm1.serialize() == P + kNm1);
    CHECK(odd.serialize() == P + "0ABC");
    CHECK(HipP256PrivateKey(one.serialize()).serialize() == one.serialize());
    CHECK(HipP256PrivateKey(odd.serialize()).publicKeySerialized() == odd.publicKeySerialized());
    CHECK(lower.publicKeySerialized() == kRfcPub);
    // RFC 6979 A.2.5, "sample": the DER form of its r, s (both have the top bit set)
    CHECK(hexOf(lower.sign("sample")) ==
          "3046022100efd48b2aacb6a8fd1140dd9cd45e81d69d2c877b56aaf991c34d0ea84eaf3716"
          "022100f7cb1c942d657c41d436c7a1b6e29f65f3e900dbb9aff4064dc4ab2f843acda8");
    // "test": s has its top bit clear and takes no padding byte
    CHECK(hexOf(lower.sign("test")) ==
          "3045022100f1abb023518351cd71d881567b1ea663ed3efcf6c5132b354f28d3b0b7d38367"
          "0220019f4113742a2b14bd25926b49c649155f267e60d3814b4c0cc84250e46f0083");
  }

  const SignStats s0 = ecdsaP256SignStats();
  std::vector<std::unique_ptr<HipP256PrivateKey>> keys;
  keys.emplace_back(new HipP256PrivateKey(P + kRfcX));
  keys.emplace_back(new HipP256PrivateKey(P + "7F" + std::string(60, '5') + "01"));
  std::vector<EVP_PKEY*> ossl;
  std::vector<std::unique_ptr<HipP256PublicKey>> pubs;
  for (auto& k : keys) {
    ossl.push_back(opensslKey(k->publicKeySerialized()));
    pubs.emplace_back(new HipP256PublicKey(k->publicKeySerialized()));
  }

  // sign(): accepted by EVP_DigestVerify and by HipP256PublicKey; a changed message is not
  for (size_t i = 0; i < 12; i++) {
    const std::string m = message(i * 11);
    const std::string der = keys[i & 1]->sign(m);
    CHECK(der == keys[i & 1]->sign(m));  // deterministic
    CHECK(opensslVerifyDer(ossl[i & 1], m, der));
    CHECK(!opensslVerifyDer(ossl[i & 1], m + "x", der));
    CHECK(!opensslVerifyDer(ossl[(i & 1) ^ 1], m, der));
    if (i < 4) CHECK(pubs[i & 1]->verify(m, der) && !pubs[i & 1]->verify(m + "x", der));
  }

  // signBatch of one key, byte for byte the sign() loop
  const size_t n = 90;
  std::vector<std::string> msgs(n), got(n);
  std::vector<HipP256PrivateKey::Request> reqs;
  for (size_t i = 0; i < n; i++) {
    msgs[i] = message(i);
    reqs.push_back({keys[0].get(), msgs[i].data(), msgs[i].size(), &got[i]});
  }
  HipP256PrivateKey::signBatch(reqs);
  for (size_t i = 0; i < n; i++) CHECK(got[i] == keys[0]->sign(msgs[i]));
  const SignStats s1 = ecdsaP256SignStats();
  if (on_gpu) {
    CHECK(s1.gpu_batches == s0.gpu_batches + 1 && s1.gpu_items == s0.gpu_items + n && s1.host_items == s0.host_items);
  } else {
    CHECK(s1.gpu_batches == s0.gpu_batches && s1.gpu_items == s0.gpu_items && s1.host_items == s0.host_items + n);
  }
  CHECK(s1.gpu_errors == s0.gpu_errors);

  // a batch mixing two keys, with an empty message, a skipped request (null key) and a lone trailing one
  std::vector<std::string> got2(n + 1);
  reqs.clear();
  msgs[3].clear();
  for (size_t i = 0; i < n; i++) reqs.push_back({keys[i % 3 == 0 ? 1 : 0].get(), msgs[i].data(), msgs[i].size(), &got2[i]});
  got2[n] = "untouched";
  reqs.push_back({nullptr, msgs[0].data(), msgs[0].size(), &got2[n]});
  HipP256PrivateKey::signBatch(reqs);
  for (size_t i = 0; i < n; i++) {
    const size_t k = i % 3 == 0 ? 1 : 0;
    CHECK(got2[i] == keys[k]->sign(msgs[i]));
    if (i % 9 == 0) CHECK(opensslVerifyDer(ossl[k], msgs[i], got2[i]) && pubs[k]->verify(msgs[i], got2[i]));
  }
  CHECK(got2[n] == "untouched");
  const SignStats s2 = ecdsaP256SignStats();
  if (on_gpu) {  // one GPU call per key
    CHECK(s2.gpu_batches == s1.gpu_batches + 2 && s2.gpu_items == s1.gpu_items + n && s2.host_items == s1.host_items);
  } else {
    CHECK(s2.gpu_batches == s1.gpu_batches && s2.host_items == s1.host_items + n);
  }
  CHECK(s2.gpu_errors == s0.gpu_errors);

  // a lone request, and an empty batch
  std::string lone;
  std::vector<HipP256PrivateKey::Request> r1{{keys[1].get(), msgs[7].data(), msgs[7].size(), &lone}}, r0;
  HipP256PrivateKey::signBatch(r1);
  HipP256PrivateKey::signBatch(r0);
  CHECK(lone == keys[1]->sign(msgs[7]));
  const SignStats s3 = ecdsaP256SignStats();
  CHECK(on_gpu ? (s3.gpu_batches == s2.gpu_batches + 1 && s3.gpu_items == s2.gpu_items + 1)
               : (s3.host_items == s2.host_items + 1 && s3.gpu_batches == s2.gpu_batches));

  // a key that goes away unloads its table; one made afterwards from the same scalar signs the same bytes
  keys[0].reset();
  HipP256PrivateKey again(P + kRfcX);
  std::string a2;
  std::vector<HipP256PrivateKey::Request> r2{{&again, msgs[5].data(), msgs[5].size(), &a2}};
  HipP256PrivateKey::signBatch(r2);
  CHECK(a2 == got[5] && a2 == again.sign(msgs[5]));

  for (EVP_PKEY* k : ossl) EVP_PKEY_free(k);
}

int main(int argc, char** argv) {
  const bool no_gpu = argc > 1 && std::strcmp(argv[1], "--no-gpu") == 0;
  // read once, at the first signBatch; the verify side stays on the host in both modes
  setenv("CBFT_ECDSA_P256_SIGN_GPU_MIN", no_gpu ? "1000000" : "1", 1);
  setenv("CBFT_ECDSA_P256_GPU_MIN", "1000000", 1);
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
