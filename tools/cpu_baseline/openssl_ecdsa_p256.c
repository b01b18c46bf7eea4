/* Host-CPU ECDSA P-256 (prime256v1) / SHA-256 baseline of tools/ecdsa_p256_bench.py: OpenSSL SHA256 +
 * ECDSA_do_verify on NID_X9_62_prime256v1, success only on == 1, one EC_KEY cached per public key (as one
 * verifier object is kept per key), T pthreads over static contiguous ranges.  Also signs (the benchmark's
 * inputs).  Never linked into libcbft_hipcrypto. */
#include <openssl/bn.h>
#include <openssl/ec.h>
#include <openssl/ecdsa.h>
#include <openssl/obj_mac.h>
#include <openssl/sha.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* Opaque key cache for nkeys 64-byte public keys (X || Y big-endian); a key OpenSSL refuses is NULL. */
void* cbft_cpu_p256_keys_new(const uint8_t* pub, uint32_t nkeys) {
  EC_KEY** keys = (EC_KEY**)calloc(nkeys ? nkeys : 1, sizeof(EC_KEY*));
  for (uint32_t i = 0; i < nkeys; i++) {
    EC_KEY* k = EC_KEY_new_by_curve_name(NID_X9_62_prime256v1);
    BIGNUM* x = BN_bin2bn(pub + 64 * (size_t)i, 32, NULL);
    BIGNUM* y = BN_bin2bn(pub + 64 * (size_t)i + 32, 32, NULL);
    if (k && EC_KEY_set_public_key_affine_coordinates(k, x, y) == 1) {
      keys[i] = k;
    } else {
      EC_KEY_free(k);
    }
    BN_free(x);
    BN_free(y);
  }
  return keys;
}
void cbft_cpu_p256_keys_free(void* h, uint32_t nkeys) {
  EC_KEY** keys = (EC_KEY**)h;
  for (uint32_t i = 0; i < nkeys; i++) EC_KEY_free(keys[i]);
  free(keys);
}

typedef struct {
  EC_KEY** keys;
  const uint32_t* key_idx;
  const uint8_t* sig;
  const uint8_t* blob;
  const uint64_t* off;
  const uint32_t* len;
  size_t lo, hi;
  uint8_t* out;
} job_t;

static void* worker(void* arg) {
  job_t* j = (job_t*)arg;
  for (size_t i = j->lo; i < j->hi; i++) {
    EC_KEY* k = j->keys[j->key_idx[i]];
    int ok = 0;
    if (k) {
      uint8_t dg[32];
      SHA256(j->blob + j->off[i], j->len[i], dg);
      ECDSA_SIG* s = ECDSA_SIG_new();
      BIGNUM* r = BN_bin2bn(j->sig + 64 * i, 32, NULL);
      BIGNUM* v = BN_bin2bn(j->sig + 64 * i + 32, 32, NULL);
      if (s && r && v && ECDSA_SIG_set0(s, r, v) == 1) {
        ok = ECDSA_do_verify(dg, 32, s, k) == 1;
      } else {
        BN_free(r);
        BN_free(v);
      }
      ECDSA_SIG_free(s);
    }
    j->out[i] = (uint8_t)ok;
  }
  return NULL;
}

/* Verify n signatures (r || s, 64 bytes each) on `threads` threads; out[i] = 0/1. */
int cbft_cpu_p256_verify(void* keycache, const uint32_t* key_idx, const uint8_t* sig, const uint8_t* blob,
                          const uint64_t* off, const uint32_t* len, size_t n, uint8_t* out, int threads) {
  if (threads < 1) threads = 1;
  pthread_t* th = (pthread_t*)calloc(threads, sizeof(pthread_t));
  job_t* jobs = (job_t*)calloc(threads, sizeof(job_t));
  for (int t = 0; t < threads; t++) {
    jobs[t] = (job_t){(EC_KEY**)keycache, key_idx, sig, blob, off, len, n * t / threads, n * (t + 1) / threads, out};
    pthread_create(&th[t], NULL, worker, &jobs[t]);
  }
  for (int t = 0; t < threads; t++) pthread_join(th[t], NULL);
  free(th);
  free(jobs);
  return 0;
}

/* nkeys fresh key pairs: priv = nkeys x 32 bytes, pub = nkeys x 64 bytes. */
int cbft_cpu_p256_keygen(uint32_t nkeys, uint8_t* priv, uint8_t* pub) {
  for (uint32_t i = 0; i < nkeys; i++) {
    EC_KEY* k = EC_KEY_new_by_curve_name(NID_X9_62_prime256v1);
    if (!k || EC_KEY_generate_key(k) != 1) return -1;
    BIGNUM *x = BN_new(), *y = BN_new();
    if (EC_POINT_get_affine_coordinates(EC_KEY_get0_group(k), EC_KEY_get0_public_key(k), x, y, NULL) != 1) return -1;
    BN_bn2binpad(EC_KEY_get0_private_key(k), priv + 32 * (size_t)i, 32);
    BN_bn2binpad(x, pub + 64 * (size_t)i, 32);
    BN_bn2binpad(y, pub + 64 * (size_t)i + 32, 32);
    BN_free(x);
    BN_free(y);
    EC_KEY_free(k);
  }
  return 0;
}

typedef struct {
  EC_KEY** keys;
  const uint32_t* key_idx;
  const uint8_t* blob;
  const uint64_t* off;
  const uint32_t* len;
  size_t lo, hi;
  uint8_t* sig;
  int rc;
} sjob_t;

static void* sworker(void* arg) {
  sjob_t* j = (sjob_t*)arg;
  for (size_t i = j->lo; i < j->hi; i++) {
    uint8_t dg[32];
    SHA256(j->blob + j->off[i], j->len[i], dg);
    ECDSA_SIG* s = ECDSA_do_sign(dg, 32, j->keys[j->key_idx[i]]);
    if (!s) {
      j->rc = -1;
      return NULL;
    }
    BN_bn2binpad(ECDSA_SIG_get0_r(s), j->sig + 64 * i, 32);
    BN_bn2binpad(ECDSA_SIG_get0_s(s), j->sig + 64 * i + 32, 32);
    ECDSA_SIG_free(s);
  }
  return NULL;
}

/* Sign n messages (sig = n x 64 bytes, r || s) with the keys priv[key_idx[i]] on `threads` threads. */
int cbft_cpu_p256_sign_many(const uint8_t* priv, uint32_t nkeys, const uint32_t* key_idx, const uint8_t* blob,
                             const uint64_t* off, const uint32_t* len, size_t n, uint8_t* sig, int threads) {
  EC_KEY** keys = (EC_KEY**)calloc(nkeys ? nkeys : 1, sizeof(EC_KEY*));
  for (uint32_t i = 0; i < nkeys; i++) {
    keys[i] = EC_KEY_new_by_curve_name(NID_X9_62_prime256v1);
    BIGNUM* d = BN_bin2bn(priv + 32 * (size_t)i, 32, NULL);
    EC_KEY_set_private_key(keys[i], d);
    BN_free(d);
  }
  if (threads < 1) threads = 1;
  pthread_t* th = (pthread_t*)calloc(threads, sizeof(pthread_t));
  sjob_t* jobs = (sjob_t*)calloc(threads, sizeof(sjob_t));
  for (int t = 0; t < threads; t++) {
    jobs[t] = (sjob_t){keys, key_idx, blob, off, len, n * t / threads, n * (t + 1) / threads, sig, 0};
    pthread_create(&th[t], NULL, sworker, &jobs[t]);
  }
  int rc = 0;
  for (int t = 0; t < threads; t++) {
    pthread_join(th[t], NULL);
    if (jobs[t].rc) rc = jobs[t].rc;
  }
  for (uint32_t i = 0; i < nkeys; i++) EC_KEY_free(keys[i]);
  free(keys);
  free(th);
  free(jobs);
  return rc;
}
