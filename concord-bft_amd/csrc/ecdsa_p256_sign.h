// Deterministic ECDSA P-256 (secp256r1) / SHA-256 batch signing: the lane routines (host and device,
// one source) and the device-side launch interface (internal to libcbft_hipcrypto; the public C ABI
// is include/cbft_hipcrypto.h).
//
// The batch form of concord::util::openssl_utils::AsymmetricPrivateKey::sign (util/src/
// openssl_crypto.cpp, EVPPKEYPrivateKey::sign: EVP_DigestSign, SHA-256, prime256v1).  OpenSSL draws
// k at random; here k is the RFC 6979 nonce, so every signature is reproducible byte for byte
// (tests/p256_sign_ref.py).  The scheme is ecdsa_sign.h's with the P-256 constants:
//
//   h1 = SHA-256(m);  e = h1 mod n;  k = HMAC-SHA-256 DRBG(x || bits2octets(h1)), first candidate
//   with 1 <= k < n, r != 0 and s != 0;  R = k G;  r = x(R) mod n;  s = k^-1 (e + r x) mod n.
//   The lane emits r || s as computed (no low-s rule); the DER form is the host's (ecdsa_der.h).
//
// Secret independence.  x, k, the DRBG's K and V, k^-1, every intermediate of k G (Z included) and
// e + r x enter arithmetic and mask selects only: no branch, loop bound, address or choice of load
// depends on them.  The variable-time point code of ge_p256.h (p2_ge_dbl, p2_ge_madd, p2_ge_to_aff)
// builds the PUBLIC comb table of G alone (p2s_table_lane).  The one exception is the candidate loop
// of p2s_sign_lane / ecdsas_nonce_skip: it runs again when a candidate is rejected (k = 0, k >= n,
// r = 0 or s = 0), which reveals that a rejection happened and nothing else.  Here 2^256 - n is
// about 2^224, so a first candidate k >= n has probability about 2^-32 per signature (2^-128 on
// secp256k1): in a batch of 65,536 about one batch in 65,536 holds such a lane.
//
// Additions: the complete mixed addition of Renes, Costello and Batina for a = -3 (Algorithm 5 of
// "Complete addition formulas for prime order elliptic curves") on homogeneous projective
// coordinates (x = X / Z, infinity = (0 : 1 : 0)): 11 products and 2 products by b, which is a full
// field element here, so 13 p2_fe_mul.  No exceptional case for any affine Q on the curve (the
// group order is odd); a zero digit computes a sum with Q = (0, 0) and drops it under a mask.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ecdsa_p256_verify.h"  // the field, the scalars, the variable-time point code (table only)
#include "ecdsa_sign.h"         // the DRBG, the masks, the comb's geometry, EcdsaSignBatch

// The comb table and the signer record have ecdsa_sign.h's layout: ECDSAS_TABLE_WORDS words
// (64 positions x 8 affine entries x[8] | y[8], then 2^256 G; n - 1 + 0x88..8 overflows 2^256 here
// too), and x[8] | Qx[8] | Qy[8] | validity | 7 zero words.

// ---- GF(p) additions to fe_p256.h ----------------------------------------------------------------
// r = b a
K1_HD void p2s_fe_mulb(P2Fe& r, const P2Fe& a) {
  const uint32_t B[8] = P2_B_LIMBS;
  P2Fe b;
#pragma unroll
  for (int i = 0; i < 8; i++) b.v[i] = B[i];
  p2_fe_mul(r, a, b);
}
K1_HD void p2s_fe_sqrn(P2Fe& r, const P2Fe& a, int n) {
  r = a;
#pragma unroll 1
  for (int i = 0; i < n; i++) p2_fe_sqr(r, r);
}
// r = a^(p - 2) = a^-1 (0 -> 0): a fixed chain over the bit runs of
// p - 2 = 1^32 0^31 1 0^96 1^94 0 1, 255 squarings and 12 products whatever a is.
K1_HD void p2s_fe_inv_ct(P2Fe& r, const P2Fe& a) {
  P2Fe x2, x30, x32, t;
  p2_fe_sqr(t, a);
  p2_fe_mul(x2, t, a);
  p2_fe_sqr(t, x2);
  p2_fe_mul(t, t, a);  // x3
  p2s_fe_sqrn(x30, t, 3);
  p2_fe_mul(x30, x30, t);  // x6
  p2s_fe_sqrn(x32, x30, 6);
  p2_fe_mul(x32, x32, x30);  // x12
  p2s_fe_sqrn(x32, x32, 3);
  p2_fe_mul(t, x32, t);  // x15
  p2s_fe_sqrn(x30, t, 15);
  p2_fe_mul(x30, x30, t);  // x30
  p2s_fe_sqrn(t, x30, 2);
  p2_fe_mul(x32, t, x2);  // x32
  p2s_fe_sqrn(t, x32, 32);
  p2_fe_mul(t, t, a);  // 1^32 0^31 1
  p2s_fe_sqrn(t, t, 96 + 32);
  p2_fe_mul(t, t, x32);
  p2s_fe_sqrn(t, t, 32);
  p2_fe_mul(t, t, x32);
  p2s_fe_sqrn(t, t, 30);
  p2_fe_mul(t, t, x30);  // .. 1^94
  p2s_fe_sqrn(t, t, 2);
  p2_fe_mul(r, t, a);
}

// ---- arithmetic mod n additions to sc_p256.h -----------------------------------------------------
// r = a^-1 2^256 mod n (the Montgomery residue of the inverse; 0 -> 0), a < n: square and multiply
// over the bits of the PUBLIC exponent n - 2 (the same 255 squarings and products whatever a is).
// The exponent shifts through eight words at compile-time indices.
K1_HD void p2s_sc_inv_mont(P2Sc& r, const P2Sc& a) {
  uint32_t ex[8] = P2_N_LIMBS;
  ex[0] -= 2u;
  P2Sc am, acc;
  p2_sc_to_mont(am, a);
  acc = am;  // bit 255 of n - 2 is set
#pragma unroll 1
  for (int bit = 254; bit >= 0; bit--) {
#pragma unroll
    for (int j = 7; j > 0; j--) ex[j] = (ex[j] << 1) | (ex[j - 1] >> 31);
    ex[0] <<= 1;
    p2_sc_montmul(acc, acc.v, acc.v);
    if (ex[7] >> 31) p2_sc_montmul(acc, acc.v, am.v);  // a bit of n - 2: public
  }
  r = acc;
}
// r = a^-1 mod n (0 -> 0), a < n
K1_HD void p2s_sc_inv_ct(P2Sc& r, const P2Sc& a) {
  P2Sc m;
  p2s_sc_inv_mont(m, a);
  uint32_t one[8];
#pragma unroll
  for (int i = 0; i < 8; i++) one[i] = i == 0 ? 1u : 0u;
  p2_sc_montmul(r, one, m.v);
}
// r = a + b mod n, a, b < n
K1_HD void p2s_sc_add_ct(P2Sc& r, const P2Sc& a, const P2Sc& b) {
  const uint32_t N[8] = P2_N_LIMBS;
  uint32_t t[8], u[8];
  const uint32_t carry = k1_add256(t, a.v, b.v);
  const uint32_t borrow = k1_sub256(u, t, N);
  const uint32_t take = 0u - (carry | (borrow ^ 1u));
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = k1s_pick(take, u[i], t[i]);
}
// r = x mod n for a field element x (< p < 2 n): one masked subtraction.  p - n < 2^128, so no
// nonce anyone can find reaches x(R) >= n: only a direct test exercises the subtraction.
K1_HD void p2s_x_mod_n(P2Sc& r, const P2Fe& x) {
  const uint32_t N[8] = P2_N_LIMBS;
  k1s_reduce_once(r.v, x.v, N);
}

// ---- points: homogeneous projective, complete mixed addition ------------------------------------
struct P2Proj {
  P2Fe x, y, z;
};
K1_HD void p2s_set_inf(P2Proj& r) {
  p2_fe_zero(r.x);
  p2_fe_one(r.y);
  p2_fe_zero(r.z);
}
// r = p + q for any p (infinity included) and any affine q on the curve: 13 products, no case split
K1_HD void p2s_madd(P2Proj& r, const P2Proj& p, const P2Fe& qx, const P2Fe& qy) {
  P2Fe t0, t1, t2, t3, t4, x3, y3, z3;
  p2_fe_mul(t0, p.x, qx);
  p2_fe_mul(t1, p.y, qy);
  p2_fe_add(t3, qx, qy);
  p2_fe_add(t4, p.x, p.y);
  p2_fe_mul(t3, t3, t4);
  p2_fe_add(t4, t0, t1);
  p2_fe_sub(t3, t3, t4);
  p2_fe_mul(t4, qy, p.z);
  p2_fe_add(t4, t4, p.y);
  p2_fe_mul(y3, qx, p.z);
  p2_fe_add(y3, y3, p.x);
  p2s_fe_mulb(z3, p.z);
  p2_fe_sub(x3, y3, z3);
  p2_fe_add(z3, x3, x3);
  p2_fe_add(x3, x3, z3);
  p2_fe_sub(z3, t1, x3);
  p2_fe_add(x3, t1, x3);
  p2s_fe_mulb(y3, y3);
  p2_fe_add(t1, p.z, p.z);
  p2_fe_add(t2, t1, p.z);
  p2_fe_sub(y3, y3, t2);
  p2_fe_sub(y3, y3, t0);
  p2_fe_add(t1, y3, y3);
  p2_fe_add(y3, t1, y3);
  p2_fe_add(t1, t0, t0);
  p2_fe_add(t0, t1, t0);
  p2_fe_sub(t0, t0, t2);
  p2_fe_mul(t1, t4, y3);
  p2_fe_mul(t2, t0, y3);
  p2_fe_mul(y3, x3, z3);
  p2_fe_add(r.y, y3, t2);
  p2_fe_mul(x3, t3, x3);
  p2_fe_sub(r.x, x3, t1);
  p2_fe_mul(z3, t4, z3);
  p2_fe_mul(t1, t3, t0);
  p2_fe_add(r.z, z3, t1);
}
// r = m ? a : r
K1_HD void p2s_cmov(P2Proj& r, const P2Proj& a, uint32_t m) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    r.x.v[i] = k1s_pick(m, a.x.v[i], r.x.v[i]);
    r.y.v[i] = k1s_pick(m, a.y.v[i], r.y.v[i]);
    r.z.v[i] = k1s_pick(m, a.z.v[i], r.z.v[i]);
  }
}

// P = k G for ANY 256-bit k (0 and n give infinity): ecdsas_comb's shape.  Every lane reads all 8
// entries of every position (addresses depend on j and e only) and keeps one under a mask; the sign
// is applied by a select; a zero digit computes a sum and drops it.  65 additions, no doubling.
K1_HD void p2s_comb(P2Proj& P, const uint32_t* k, const uint32_t* __restrict__ tbl) {
  uint32_t t[8];
  uint32_t carry;
  {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      c += (uint64_t)k[i] + 0x88888888u;
      t[i] = (uint32_t)c;
      c >>= 32;
    }
    carry = (uint32_t)c;
  }
  p2s_set_inf(P);
  {
    P2Fe qx, qy;
    const uint32_t* q = tbl + ECDSAS_TOP_WORD;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      qx.v[i] = q[i];
      qy.v[i] = q[8 + i];
    }
    P2Proj S;
    p2s_madd(S, P, qx, qy);
    p2s_cmov(P, S, k1s_opaque(0u - carry));
  }
#pragma unroll 1
  for (int j = ECDSAS_NPOS - 1; j >= 0; j--) {
    // the digit is the top nibble, which then moves out (limbs stay at compile-time indices)
    const int32_t d = (int32_t)(t[7] >> 28) - 8;  // [-8, 7]
#pragma unroll
    for (int i = 7; i > 0; i--) t[i] = (t[i] << 4) | (t[i - 1] >> 28);
    t[0] <<= 4;
    const uint32_t sgn = (uint32_t)(d >> 31);        // all ones when negative
    const uint32_t mag = ((uint32_t)d ^ sgn) - sgn;  // 0..8
    P2Fe qx, qy;
    p2_fe_zero(qx);
    p2_fe_zero(qy);
    const uint32_t* pos = tbl + (size_t)j * (ECDSAS_ENTRIES * 16);
#pragma unroll
    for (int e = 1; e <= ECDSAS_ENTRIES; e++) {
      const uint32_t* q = pos + (e - 1) * 16;
      // mag ^ e is 0 on a hit and 1..15 otherwise: minus one is negative on a hit alone
      const uint32_t hit = k1s_opaque((uint32_t)((int32_t)((mag ^ (uint32_t)e) - 1u) >> 31));
#pragma unroll
      for (int i = 0; i < 8; i++) {
        qx.v[i] = k1s_pick(hit, q[i], qx.v[i]);
        qy.v[i] = k1s_pick(hit, q[8 + i], qy.v[i]);
      }
    }
    P2Fe ny;
    p2_fe_neg(ny, qy);
    const uint32_t neg = k1s_opaque(sgn);
#pragma unroll
    for (int i = 0; i < 8; i++) qy.v[i] = k1s_pick(neg, ny.v[i], qy.v[i]);
    P2Proj S;
    p2s_madd(S, P, qx, qy);  // digit 0: Q = (0, 0), the sum is dropped
    p2s_cmov(P, S, k1s_opaque(0u - ((mag | (0u - mag)) >> 31)));
  }
}

// Table lane j: the multiples 1..8 of 16^j G (j < 64) or 2^256 G (j = 64), affine.  Public data,
// once per context: the verify path's variable-time point code.
K1_HD void p2s_table_lane(uint32_t* tbl, int j) {
  const uint8_t g[64] = ECDSA_P256_G_BYTES;
  P2Aff base;
  (void)p2_fe_from_be(base.x, g);
  (void)p2_fe_from_be(base.y, g + 32);
  P2Jac a;
  p2_ge_from_aff(a, base);
#pragma unroll 1
  for (int i = 0; i < 4 * j; i++) p2_ge_dbl(a, a);
  p2_ge_to_aff(base, a);
  uint32_t* o = j < ECDSAS_NPOS ? tbl + (size_t)j * (ECDSAS_ENTRIES * 16) : tbl + ECDSAS_TOP_WORD;
  const int entries = j < ECDSAS_NPOS ? ECDSAS_ENTRIES : 1;
  p2_ge_from_aff(a, base);
#pragma unroll 1
  for (int e = 1; e <= entries; e++) {
    P2Aff q = base;
    if (e > 1) {
      p2_ge_madd(a, a, base);  // e = 2 is the doubling branch
      p2_ge_to_aff(q, a);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      o[(e - 1) * 16 + i] = q.x.v[i];
      o[(e - 1) * 16 + 8 + i] = q.y.v[i];
    }
  }
}

// ---- one signature -------------------------------------------------------------------------------
// r, s for the nonce k (1 <= k < n), the key x (< n) and the reduced digest e (< n); all ones
// unless r = 0 or s = 0
K1_HD uint32_t p2s_sign_with_k(P2Sc& r, P2Sc& s, const uint32_t* x, const P2Sc& e, const uint32_t* k,
                               const uint32_t* __restrict__ tbl) {
  P2Proj R;
  p2s_comb(R, k, tbl);
  P2Fe zi, xa;
  p2s_fe_inv_ct(zi, R.z);
  p2_fe_mul(xa, R.x, zi);
  p2s_x_mod_n(r, xa);
  P2Sc kk, kim, xm, t;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    kk.v[i] = k[i];
    xm.v[i] = x[i];
  }
  p2s_sc_inv_mont(kim, kk);         // k^-1 2^256
  p2_sc_to_mont(xm, xm);            // x 2^256
  p2_sc_montmul(t, r.v, xm.v);      // r x
  p2s_sc_add_ct(t, t, e);           // e + r x
  p2_sc_montmul(s, t.v, kim.v);     // k^-1 (e + r x)
  return k1s_nonzero_mask(r.v) & k1s_nonzero_mask(s.v);
}
// sig[0..16): r || s as big-endian words in memory order (sig[i] holds bytes 4 i .. 4 i + 3)
K1_HD void p2s_put_sig(uint32_t* sig, const P2Sc& r, const P2Sc& s) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    sig[i] = __builtin_bswap32(r.v[7 - i]);
    sig[8 + i] = __builtin_bswap32(s.v[7 - i]);
  }
}
// One signature under a usable key x (1 <= x < n): h1 = the digest's big-endian words (it seeds the
// generator), e = the reduced digest that enters s.  The product passes e = h1 mod n (p2s_sign_lane);
// a test passes another e to reach the s = 0 retry, which no message does.
K1_HD void p2s_sign_lane_e(uint32_t* sig, const uint32_t* x, const uint32_t* h1, const P2Sc& e,
                           const uint32_t* __restrict__ tbl) {
  const uint32_t N[8] = P2_N_LIMBS;
  P2Sc r, s;
#pragma unroll 1
  for (uint32_t skip = 0;; skip++) {
    // r = 0 or s = 0 (probability about 2^-255): the generator is run again from its start and
    // passes over the candidates already refused, so no DRBG state is alive across the signature
    uint32_t k[8];
    (void)ecdsas_nonce_skip(k, x, h1, N, skip);
    if (p2s_sign_with_k(r, s, x, e, k, tbl)) break;
  }
  p2s_put_sig(sig, r, s);
}
K1_HD void p2s_sign_lane(uint32_t* sig, const uint32_t* x, const uint32_t* h1, const uint32_t* __restrict__ tbl) {
  uint32_t z[8];
#pragma unroll
  for (int i = 0; i < 8; i++) z[i] = h1[7 - i];
  P2Sc e;
  p2_sc_reduce256(e, z);
  p2s_sign_lane_e(sig, x, h1, e, tbl);
}

// Signer record from 32 big-endian bytes: x = 0 or x >= n gets a zero record (validity clear).
K1_HD void p2s_signer_lane(uint32_t* rec, const uint8_t* priv, const uint32_t* __restrict__ tbl) {
  const uint32_t N[8] = P2_N_LIMBS;
  uint32_t x[8];
  k1_from_be(x, priv);
  const uint32_t ok = k1s_opaque(k1s_nonzero_mask(x) & k1s_lt_mask(x, N));
#pragma unroll
  for (int i = 0; i < 8; i++) x[i] &= ok;
  P2Proj Q;
  p2s_comb(Q, x, tbl);  // x = 0: infinity, Z = 0, whose "inverse" is 0: Q = (0, 0)
  P2Fe zi, qx, qy;
  p2s_fe_inv_ct(zi, Q.z);
  p2_fe_mul(qx, Q.x, zi);
  p2_fe_mul(qy, Q.y, zi);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    rec[i] = x[i];
    rec[8 + i] = qx.v[i] & ok;
    rec[16 + i] = qy.v[i] & ok;
    rec[24 + i] = i == 0 ? (ok & 1u) : 0u;
  }
}

#if defined(__HIPCC__)
// The launch interface mirrors ecdsa_sign.h's: the same EcdsaSignBatch, the same scratch layout
// (cbft_ecdsa_sign_scratch_words) and the same zero output for an unusable signer.
hipError_t cbft_ecdsa_p256_sign_build_table(uint32_t* d_tbl, hipStream_t stream);
hipError_t cbft_ecdsa_p256_sign_launch_keys(const uint8_t* d_priv, uint32_t nkeys, const uint32_t* d_tbl,
                                            uint32_t* d_signers, hipStream_t stream);
hipError_t cbft_ecdsa_p256_sign_launch(const EcdsaSignBatch& b, const uint32_t* d_tbl, uint32_t* d_scratch,
                                       uint8_t* d_sig, hipStream_t stream);
#endif
