// ECDSA P-256 (secp256r1) / SHA-256 batch verification: the lane routines (host and device, one
// source) and the device-side launch interface (internal to libcbft_hipcrypto; the public C ABI is
// include/cbft_hipcrypto.h).
//
// Reference behaviour: concord::util::openssl_utils::AsymmetricPublicKey (util/src/
// openssl_crypto.cpp) = OpenSSL EVP on secp256r1 with SHA-256; verdicts pinned to OpenSSL 3.0.2
// ECDSA_do_verify by tests/golden/ecdsa_p256_vectors.json and restated in tests/p256_ref.py.  The
// DER form of the signature is undone on the host (ecdsa_der.h); here a signature is r || s.
//
//   accept iff  the key is on the curve (X, Y < p),  1 <= r, s < n,
//               R = u1 G + u2 Q != infinity  with  w = s^-1, u1 = e w, u2 = r w (mod n),
//               e = SHA-256(m) as an integer,  and  x(R) mod n == r.
//
// The scheme is ecdsa_verify.h's: Straus 4-bit windows over the affine multiples 1..15 of G and
// of Q, every addition a p2_ge_madd with its three exceptional branches, and the closing test on
// the Jacobian R without an inversion: accept iff r Z^2 == X or (r + n < p and (r + n) Z^2 == X).
// p - n < 2^127 here, so the second arm needs r < 2^127.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ecdsa_verify.h"  // the key record's layout, ecdsa_sha256
#include "ge_p256.h"
#include "sc_p256.h"

// the generator, X || Y big-endian
#define ECDSA_P256_G_BYTES                                                                           \
  {                                                                                                  \
    0x6B, 0x17, 0xD1, 0xF2, 0xE1, 0x2C, 0x42, 0x47, 0xF8, 0xBC, 0xE6, 0xE5, 0x63, 0xA4, 0x40, 0xF2, \
    0x77, 0x03, 0x7D, 0x81, 0x2D, 0xEB, 0x33, 0xA0, 0xF4, 0xA1, 0x39, 0x45, 0xD8, 0x98, 0xC2, 0x96, \
    0x4F, 0xE3, 0x42, 0xE2, 0xFE, 0x1A, 0x7F, 0x9B, 0x8E, 0xE7, 0xEB, 0x4A, 0x7C, 0x0F, 0x9E, 0x16, \
    0x2B, 0xCE, 0x33, 0x57, 0x6B, 0x31, 0x5E, 0xCE, 0xCB, 0xB6, 0x40, 0x68, 0x37, 0xBF, 0x51, 0xF5  \
  }

K1_HD void ecdsa_p256_load_aff(P2Aff& a, const uint32_t* tbl, uint32_t k /* 1..15 */) {
  const uint32_t* q = tbl + (size_t)(k - 1) * 16;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    a.x.v[i] = q[i];
    a.y.v[i] = q[8 + i];
  }
}

// Build one key's record (the layout of ECDSA_KEY_WORDS) from its 64 bytes (X || Y big-endian).
// An unusable key (a coordinate >= p, or off the curve, which covers (0, 0)) gets a zero record
// with the validity word clear.  (0, +-sqrt(b)) is on the curve and usable.
K1_HD void ecdsa_p256_key_lane(uint32_t* rec, const uint8_t* pub) {
  P2Aff q;
  const bool inx = p2_fe_from_be(q.x, pub), iny = p2_fe_from_be(q.y, pub + 32);
  const bool ok = inx && iny && p2_ge_on_curve(q);
  if (!ok) {
    for (int i = 0; i < ECDSA_KEY_WORDS; i++) rec[i] = 0;
    return;
  }
  P2Jac acc;
  p2_ge_from_aff(acc, q);
#pragma unroll 1
  for (uint32_t k = 1; k <= ECDSA_TBL_ENTRIES; k++) {
    P2Aff a;
    if (k == 1) {
      a = q;
    } else {
      p2_ge_madd(acc, acc, q);  // k = 2 is the doubling branch; k Q != infinity for k < n
      p2_ge_to_aff(a, acc);
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
K1_HD bool ecdsa_p256_verify_lane(const uint32_t* key, const uint32_t* gtab, const uint8_t* sig, const uint32_t* h) {
  if (!key[ECDSA_KEY_OK]) return false;
  P2Sc r, s, e, w, u1, u2;
  k1_from_be(r.v, sig);
  k1_from_be(s.v, sig + 32);
  if (p2_sc_is_zero(r) || p2_sc_is_zero(s) || !p2_sc_in_range(r.v) || !p2_sc_in_range(s.v)) return false;
  uint32_t eraw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) eraw[i] = h[7 - i];
  p2_sc_reduce256(e, eraw);
  p2_sc_inv_var(w, s);
  p2_sc_to_mont(w, w);  // w 2^256: the two products below come out in plain form
  p2_sc_montmul(u1, e.v, w.v);
  p2_sc_montmul(u2, r.v, w.v);

  P2Jac acc;
  p2_ge_set_inf(acc);
#pragma unroll 1
  for (int i = 63; i >= 0; i--) {
    if (!p2_ge_is_inf(acc)) {
#pragma unroll 1
      for (int k = 0; k < 4; k++) p2_ge_dbl(acc, acc);
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
        P2Aff a;
        ecdsa_p256_load_aff(a, tbl, d);
        p2_ge_madd(acc, acc, a);
      }
    }
  }
  if (p2_ge_is_inf(acc)) return false;

  const uint32_t N[8] = P2_N_LIMBS;
  P2Fe zz, rf, t;
  p2_fe_sqr(zz, acc.z);
#pragma unroll
  for (int i = 0; i < 8; i++) rf.v[i] = r.v[i];  // r < n < p
  p2_fe_mul(t, rf, zz);
  if (p2_fe_eq(t, acc.x)) return true;
  P2Fe rn;
  if (k1_add256(rn.v, r.v, N)) return false;  // r + n >= 2^256 > p
  {
    const uint32_t P[8] = P2_P_LIMBS;
    uint32_t u[8];
    if (!k1_sub256(u, rn.v, P)) return false;  // r + n >= p
  }
  p2_fe_mul(t, rn, zz);
  return p2_fe_eq(t, acc.x);
}

#if defined(__HIPCC__)
// Validate nkeys keys (64 B each) and build their records.
hipError_t cbft_ecdsa_p256_launch_keys(const uint8_t* d_pub, uint32_t nkeys, uint32_t* d_keys, hipStream_t stream);
// Hash, then verify; writes ceil(n/64) verdict words.  d_scratch: cbft_ecdsa_scratch_words(n) words
// (the digests).  The batch is EcdsaBatch of ecdsa_verify.h with P-256 records in keys and gtab.
hipError_t cbft_ecdsa_p256_launch_verify(const EcdsaBatch& b, uint32_t* d_scratch, uint64_t* d_verdicts,
                                         hipStream_t stream);
#endif
