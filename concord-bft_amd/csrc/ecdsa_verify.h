// ECDSA secp256k1 / SHA-256 batch verification: the lane routines (host and device, one source)
// and the device-side launch interface (internal to libcbft_hipcrypto; the public C ABI is
// include/cbft_hipcrypto.h).
//
// Reference behaviour: concord::util::crypto::ECDSAVerifier (util/src/crypto_utils.cpp:34-64) =
// Crypto++ ECDSA<ECP, SHA256> on secp256k1; verdicts pinned to OpenSSL 3.0.2 ECDSA_do_verify by
// tests/golden/ecdsa_vectors.json and restated in tests/ecdsa_ref.py.
//
//   accept iff  the key is on the curve (X, Y < p),  1 <= r, s < n,
//               R = u1 G + u2 Q != infinity  with  w = s^-1, u1 = e w, u2 = r w (mod n),
//               e = SHA-256(m) as an integer,  and  x(R) mod n == r.
//
// The last test runs on the Jacobian R = (X, Y, Z) without an inversion: x(R) = X / Z^2 is r or,
// when r + n < p, r + n, so accept iff r Z^2 == X or (r + n < p and (r + n) Z^2 == X) (mod p).
//
// Scalar multiplication: interleaved (Straus) fixed windows of 4 bits over two tables of the
// affine multiples 1..15 of G and of Q: per window 4 doublings and at most one mixed addition
// from each table (a zero digit adds nothing).  Every addition is ge_madd, which tests for
// infinity, equal and opposite operands (ge_secp256k1.h), so crafted u1, u2, Q that steer the
// accumulator onto +-(a table entry) are computed correctly rather than excluded by argument.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ge_secp256k1.h"
#include "sc_secp256k1.h"
#include "sha256.h"

// Key record in HBM (uint32 words): the affine multiples k Q, k = 1..15, as x[8] | y[8]
// (little-endian limbs), then the validity word.  G's table is the record of the key Q = G.
#define ECDSA_TBL_ENTRIES 15
#define ECDSA_KEY_WORDS 256
#define ECDSA_KEY_OK 240
#define ECDSA_PUB_BYTES 64
#define ECDSA_SIG_BYTES 64

// the generator, X || Y big-endian
#define ECDSA_G_BYTES                                                                                \
  {                                                                                                  \
    0x79, 0xBE, 0x66, 0x7E, 0xF9, 0xDC, 0xBB, 0xAC, 0x55, 0xA0, 0x62, 0x95, 0xCE, 0x87, 0x0B, 0x07, \
    0x02, 0x9B, 0xFC, 0xDB, 0x2D, 0xCE, 0x28, 0xD9, 0x59, 0xF2, 0x81, 0x5B, 0x16, 0xF8, 0x17, 0x98, \
    0x48, 0x3A, 0xDA, 0x77, 0x26, 0xA3, 0xC4, 0x65, 0x5D, 0xA4, 0xFB, 0xFC, 0x0E, 0x11, 0x08, 0xA8, \
    0xFD, 0x17, 0xB4, 0x48, 0xA6, 0x85, 0x54, 0x19, 0x9C, 0x47, 0xD0, 0x8F, 0xFB, 0x10, 0xD4, 0xB8  \
  }

// One SHA-256 compression with the 64 rounds unrolled over a rolling 16-word schedule: every
// index is a compile-time constant, so state and schedule stay in registers (sha256_block of
// sha256.h keeps w[64] under run-time indices, which is 272 bytes of scratch memory per lane in a
// kernel that hashes in a loop).  blk is overwritten.
K1_HD void ecdsa_sha256_block(uint32_t* h, uint32_t* blk) {
  constexpr uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  uint32_t s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = h[i];
#pragma unroll
  for (int t = 0; t < 64; t++) {
    if (t >= 16) {
      const uint32_t w15 = blk[(t - 15) & 15], w2 = blk[(t - 2) & 15];
      const uint32_t s0 = sha256_rotr(w15, 7) ^ sha256_rotr(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = sha256_rotr(w2, 17) ^ sha256_rotr(w2, 19) ^ (w2 >> 10);
      blk[t & 15] += s0 + blk[(t - 7) & 15] + s1;
    }
    const uint32_t a = s[0], b = s[1], c = s[2], e = s[4], f = s[5], g = s[6];
    const uint32_t S1 = sha256_rotr(e, 6) ^ sha256_rotr(e, 11) ^ sha256_rotr(e, 25);
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = s[7] + S1 + ch + K[t] + blk[t & 15];
    const uint32_t S0 = sha256_rotr(a, 2) ^ sha256_rotr(a, 13) ^ sha256_rotr(a, 22);
    const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
    s[7] = g;
    s[6] = f;
    s[5] = e;
    s[4] = s[3] + t1;
    s[3] = c;
    s[2] = b;
    s[1] = a;
    s[0] = t1 + S0 + mj;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] += s[i];
}

// h[0..8) = SHA-256 state after msg[0 .. len): the digest's big-endian words.  Whole blocks are
// read straight from the message; the last one or two are assembled with the padding.
K1_HD void ecdsa_sha256(uint32_t* h, const uint8_t* msg, uint32_t len) {
  const uint32_t h0[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                          0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = h0[i];
  const uint32_t nfull = len >> 6, rem = len & 63u;
#pragma unroll 1
  for (uint32_t b = 0; b < nfull; b++) {
    uint32_t blk[16];
    const uint8_t* q = msg + (size_t)64 * b;
#pragma unroll
    for (int j = 0; j < 16; j++)
      blk[j] = ((uint32_t)q[4 * j] << 24) | ((uint32_t)q[4 * j + 1] << 16) | ((uint32_t)q[4 * j + 2] << 8) |
               q[4 * j + 3];
    ecdsa_sha256_block(h, blk);
  }
  const uint8_t* t = msg + (size_t)64 * nfull;
  const uint32_t ntail = rem + 9u > 64u ? 2u : 1u;
#pragma unroll 1
  for (uint32_t tb = 0; tb < ntail; tb++) {
    uint32_t blk[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      uint32_t w = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t pos = 64u * tb + 4u * j + k;
        const uint32_t byte = pos < rem ? t[pos] : (pos == rem ? 0x80u : 0u);
        w = (w << 8) | byte;
      }
      blk[j] = w;
    }
    if (tb == ntail - 1) {
      blk[14] = len >> 29;
      blk[15] = len << 3;
    }
    ecdsa_sha256_block(h, blk);
  }
}

K1_HD void ecdsa_load_aff(K1Aff& a, const uint32_t* tbl, uint32_t k /* 1..15 */) {
  const uint32_t* q = tbl + (size_t)(k - 1) * 16;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    a.x.v[i] = q[i];
    a.y.v[i] = q[8 + i];
  }
}

// Build one key's record from its 64 bytes (X || Y big-endian).  An unusable key (a coordinate
// >= p, or off the curve, which covers (0, 0)) gets a zero record with the validity word clear.
K1_HD void ecdsa_key_lane(uint32_t* rec, const uint8_t* pub) {
  K1Aff q;
  const bool inx = fe_from_be(q.x, pub), iny = fe_from_be(q.y, pub + 32);
  const bool ok = inx && iny && ge_on_curve(q);
  if (!ok) {
    for (int i = 0; i < ECDSA_KEY_WORDS; i++) rec[i] = 0;
    return;
  }
  K1Jac acc;
  ge_from_aff(acc, q);
#pragma unroll 1
  for (uint32_t k = 1; k <= ECDSA_TBL_ENTRIES; k++) {
    K1Aff a;
    if (k == 1) {
      a = q;
    } else {
      ge_madd(acc, acc, q);  // k = 2 is the doubling branch; k Q != infinity for k < n
      ge_to_aff(a, acc);
    }
    uint32_t* o = rec + (size_t)(k - 1) * 16;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      o[i] = a.x.v[i];
      o[8 + i] = a.y.v[i];
    }
  }
  for (int i = ECDSA_KEY_OK; i < ECDSA_KEY_WORDS; i++) rec[i] = i == ECDSA_KEY_OK ? 1u : 0u;
}

// One signature: key record, G's record, r || s (big-endian), the digest's words h[0..8).
K1_HD bool ecdsa_verify_lane(const uint32_t* key, const uint32_t* gtab, const uint8_t* sig, const uint32_t* h) {
  if (!key[ECDSA_KEY_OK]) return false;
  K1Sc r, s, e, w, u1, u2;
  k1_from_be(r.v, sig);
  k1_from_be(s.v, sig + 32);
  if (sc_is_zero(r) || sc_is_zero(s) || !sc_in_range(r.v) || !sc_in_range(s.v)) return false;
  uint32_t eraw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) eraw[i] = h[7 - i];
  sc_reduce256(e, eraw);
  sc_inv_var(w, s);
  sc_mul(u1, e, w);
  sc_mul(u2, r, w);

  K1Jac acc;
  ge_set_inf(acc);
#pragma unroll 1
  for (int i = 63; i >= 0; i--) {
    if (!ge_is_inf(acc)) {
#pragma unroll 1
      for (int k = 0; k < 4; k++) ge_dbl(acc, acc);
    }
    // the window is the top 4 bits of each scalar, which then moves up by 4 (limbs stay at
    // compile-time indices: a run-time limb index would put the scalars in scratch memory)
    const uint32_t d1 = u1.v[7] >> 28, d2 = u2.v[7] >> 28;
#pragma unroll
    for (int j = 7; j > 0; j--) {
      u1.v[j] = (u1.v[j] << 4) | (u1.v[j - 1] >> 28);
      u2.v[j] = (u2.v[j] << 4) | (u2.v[j - 1] >> 28);
    }
    u1.v[0] <<= 4;
    u2.v[0] <<= 4;
#pragma unroll 1
    for (int t = 0; t < 2; t++) {
      const uint32_t* tbl = t ? key : gtab;
      const uint32_t d = t ? d2 : d1;
      if (d) {
        K1Aff a;
        ecdsa_load_aff(a, tbl, d);
        ge_madd(acc, acc, a);
      }
    }
  }
  if (ge_is_inf(acc)) return false;

  const uint32_t N[8] = K1_N_LIMBS;
  K1Fe zz, rf, t;
  fe_sqr(zz, acc.z);
#pragma unroll
  for (int i = 0; i < 8; i++) rf.v[i] = r.v[i];  // r < n < p
  fe_mul(t, rf, zz);
  if (fe_eq(t, acc.x)) return true;
  K1Fe rn;
  if (k1_add256(rn.v, r.v, N)) return false;  // r + n >= 2^256 > p
  {
    const uint32_t P[8] = K1_P_LIMBS;
    uint32_t u[8];
    if (!k1_sub256(u, rn.v, P)) return false;  // r + n >= p
  }
  fe_mul(t, rn, zz);
  return fe_eq(t, acc.x);
}

#if defined(__HIPCC__)
// One batch, all pointers in device memory.  Signature i is sig[64 i .. 64 i + 64).
struct EcdsaBatch {
  size_t n;
  const uint32_t* keys;     // key table (ECDSA_KEY_WORDS per key)
  uint32_t nkeys;
  const uint32_t* gtab;     // G's record
  const uint32_t* key_idx;  // n indices into the key table
  const uint8_t* sig;
  const uint8_t* msg;
  const uint64_t* msg_off;
  const uint32_t* msg_len;
};
// Validate nkeys keys (64 B each) and build their records.
hipError_t cbft_ecdsa_launch_keys(const uint8_t* d_pub, uint32_t nkeys, uint32_t* d_keys, hipStream_t stream);
// Hash, then verify; writes ceil(n/64) verdict words.  d_scratch: cbft_ecdsa_scratch_words(n) words
// (the digests).
hipError_t cbft_ecdsa_launch_verify(const EcdsaBatch& b, uint32_t* d_scratch, uint64_t* d_verdicts,
                                    hipStream_t stream);
size_t cbft_ecdsa_scratch_words(size_t n);
#endif
