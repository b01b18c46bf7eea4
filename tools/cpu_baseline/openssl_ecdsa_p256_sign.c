/* Host baseline of tools/ecdsa_p256_sign_bench.py: ECDSA P-256 (prime256v1) / SHA-256 signing with
 * OpenSSL (SHA256 + ECDSA_do_sign, random nonces) on a pool of threads, with the EC_KEYs cached
 * across calls so that a timed call holds signing alone. */
#include <openssl/bn.h>
#include <openssl/ec.h>
#include <openssl/ecdsa.h>
#include <openssl/obj_mac.h>
#include <openssl/sha.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>

typedef struct {
  EC_KEY** keys;
  const uint32_t* key_idx;
  const uint8_t* blob;
  const uint64_t* off;
  const uint32_t* len;
  size_t lo, hi;
  uint8_t* sig;
  int rc;
} job_t;

static void* worker(void* arg) {
  job_t* j = (job_t*)arg;
  for (size_t i = j->lo; i < j->hi; i++) {
    uint8_t dg[32];
    SHA256(j->blob + j->off[i], j->len[i], dg);
    ECDSA_SIG* s = ECDSA_do_sign(dg, 32, j->keys[j->key_idx ? j->key_idx[i] : 0]);
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

/* The key cache: nkeys EC_KEYs from priv (32 big-endian bytes each).  NULL when a key is refused. */
void* ecdsa_p256_sign_keys_new(const uint8_t* priv, uint32_t nkeys) {
  EC_KEY** keys = (EC_KEY**)calloc(nkeys ? nkeys : 1, sizeof(EC_KEY*));
  if (!keys) return NULL;
  int bad = 0;
  for (uint32_t i = 0; i < nkeys; i++) {
    keys[i] = EC_KEY_new_by_curve_name(NID_X9_62_prime256v1);
    BIGNUM* d = BN_bin2bn(priv + 32 * (size_t)i, 32, NULL);
    if (!keys[i] || !d || EC_KEY_set_private_key(keys[i], d) != 1) bad = 1;
    BN_clear_free(d);
  }
  if (bad) {
    for (uint32_t i = 0; i < nkeys; i++) EC_KEY_free(keys[i]);
    free(keys);
    return NULL;
  }
  return keys;
}
void ecdsa_p256_sign_keys_free(void* cache, uint32_t nkeys) {
  EC_KEY** keys = (EC_KEY**)cache;
  if (!keys) return;
  for (uint32_t i = 0; i < nkeys; i++) EC_KEY_free(keys[i]);
  free(keys);
}

/* Sign n messages (sig = n x 64 bytes, r || s) with the cached keys key_idx[i] (NULL: key 0) on
 * `threads` threads.  0, or -1 when a signature could not be made. */
int ecdsa_p256_sign_many(void* cache, const uint32_t* key_idx, const uint8_t* blob, const uint64_t* off,
                         const uint32_t* len, size_t n, uint8_t* sig, int threads) {
  if (!cache) return -1;
  if (threads < 1) threads = 1;
  pthread_t* th = (pthread_t*)calloc(threads, sizeof(pthread_t));
  job_t* jobs = (job_t*)calloc(threads, sizeof(job_t));
  for (int t = 0; t < threads; t++) {
    jobs[t] = (job_t){(EC_KEY**)cache, key_idx, blob, off, len, n * t / threads, n * (t + 1) / threads, sig, 0};
    pthread_create(&th[t], NULL, worker, &jobs[t]);
  }
  int rc = 0;
  for (int t = 0; t < threads; t++) {
    pthread_join(th[t], NULL);
    if (jobs[t].rc) rc = jobs[t].rc;
  }
  free(th);
  free(jobs);
  return rc;
}
