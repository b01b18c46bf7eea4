/* Host baseline of tools/ecdsa_sign_bench.py: ECDSA secp256k1 / SHA-256 signing with OpenSSL
 * (SHA256 + ECDSA_do_sign, random nonces) on a pool of threads, EC_KEYs built once per call and
 * outside the timed part of the caller's interest only in so far as nkeys << n. */
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

/* Sign n messages (sig = n x 64 bytes, r || s) with the keys priv[key_idx[i]] (32 big-endian bytes
 * each; key_idx NULL: key 0) on `threads` threads.  0, or -1 when a signature could not be made. */
int ecdsa_sign_many(const uint8_t* priv, uint32_t nkeys, const uint32_t* key_idx, const uint8_t* blob,
                    const uint64_t* off, const uint32_t* len, size_t n, uint8_t* sig, int threads) {
  EC_KEY** keys = (EC_KEY**)calloc(nkeys ? nkeys : 1, sizeof(EC_KEY*));
  for (uint32_t i = 0; i < nkeys; i++) {
    keys[i] = EC_KEY_new_by_curve_name(NID_secp256k1);
    BIGNUM* d = BN_bin2bn(priv + 32 * (size_t)i, 32, NULL);
    EC_KEY_set_private_key(keys[i], d);
    BN_clear_free(d);
  }
  if (threads < 1) threads = 1;
  pthread_t* th = (pthread_t*)calloc(threads, sizeof(pthread_t));
  job_t* jobs = (job_t*)calloc(threads, sizeof(job_t));
  for (int t = 0; t < threads; t++) {
    jobs[t] = (job_t){keys, key_idx, blob, off, len, n * t / threads, n * (t + 1) / threads, sig, 0};
    pthread_create(&th[t], NULL, worker, &jobs[t]);
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
