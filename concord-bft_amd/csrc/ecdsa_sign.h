// Deterministic ECDSA secp256k1 / SHA-256 batch signing: the lane routines (host and device, one
// source) and the device-side launch interface (internal to libcbft_hipcrypto; the public C ABI is
// include/cbft_hipcrypto.h).
//
// The batch form of concord::util::crypto::ECDSASigner (util/src/crypto_utils.cpp:66-99): Crypto++
// ECDSA<ECP, SHA256>::Signer on secp256k1, r || s.  Crypto++ draws k at random; here k is the
// RFC 6979 nonce, so every signature is reproducible byte for byte (tests/ecdsa_sign_ref.py):
//
//   h1 = SHA-256(m);  e = h1 mod n;  k = HMAC-SHA-256 DRBG(x || bits2octets(h1)), first candidate
//   with 1 <= k < n, r != 0 and s != 0;  R = k G;  r = x(R) mod n;  s = k^-1 (e + r x) mod n.
//   s is emitted as computed (no low-s rule).
//
// Secret independence.  x, k, the DRBG's K and V, k^-1, every intermediate of k G (Z included) and
// e + r x enter arithmetic and mask selects only: no branch, loop bound, address or choice of load
// depends on them.  The verify path's helpers that break this rule (ge_madd's case split, the
// digit-indexed ecdsa_load_aff, sc_inv_var / fe_inv_var / ge_to_aff over safegcd30.h) are used for
// the PUBLIC comb table of G alone (ecdsas_table_lane).  The one exception is the candidate loop of
// ecdsas_sign_lane / ecdsas_nonce: it runs again when a candidate is rejected (k = 0, k >= n,
// r = 0 or s = 0), which reveals that a rejection happened and nothing else; for n that is an event
// of probability about 2^-128 per signature.
//
// Additions: the complete mixed addition of Renes, Costello and Batina (Algorithm 8 of "Complete
// addition formulas for prime order elliptic curves", a = 0, b3 = 21) on homogeneous projective
// coordinates (x = X / Z, infinity = (0 : 1 : 0)).  It has NO exceptional case: P = infinity,
// P = Q and P = -Q go through the same 11 products for every affine Q on the curve, because the
// group has odd order.  So no argument about which partial sums a recoding can reach is needed, at
// the top comb position (where partial sums reach the size of n) or anywhere else; the one case
// the mixed form cannot express, adding nothing (a zero digit), is taken by a mask: the sum is
// computed with whatever the scan left in Q and then dropped.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ecdsa_verify.h"

// Fixed-base comb of G in signed radix 16: k + 0x88..8 = sum_j nib_j 16^j + c 2^256, so
// k = sum_j (nib_j - 8) 16^j + c 2^256 with digits in [-8, 7] and c in {0, 1} (k reaches n - 1 >
// 2^256 - 0x88..8, so the carry is a 65th position with the single entry 2^256 G).  Position j
// (0..63) holds e * 16^j * G, e = 1..8, affine, x[8] | y[8] little-endian limbs.
#define ECDSAS_NPOS 64
#define ECDSAS_ENTRIES 8
#define ECDSAS_TOP_WORD (ECDSAS_NPOS * ECDSAS_ENTRIES * 16)
#define ECDSAS_TABLE_WORDS (ECDSAS_TOP_WORD + 16)
#define ECDSAS_TABLE_LANES (ECDSAS_NPOS + 1)
// Signer record (uint32 words): x[8] | Qx[8] | Qy[8] (little-endian limbs) | validity | 7 zero words
#define ECDSAS_WORDS 32
#define ECDSAS_OK 24
#define ECDSAS_PRIV_BYTES 32

// ---- masks ---------------------------------------------------------------------------------------
// A select mask (all ones / zero) passes through an empty asm statement before use, so that the
// compiler cannot turn the selects back into a branch around the table loads.
K1_HD uint32_t k1s_opaque(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(m));
#endif
  return m;
}
K1_HD uint32_t k1s_pick(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }  // m ? a : b
// all ones iff a != 0 (256 bits)
K1_HD uint32_t k1s_nonzero_mask(const uint32_t* a) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) x |= a[i];
  return 0u - ((x | (0u - x)) >> 31);
}
// all ones iff a < b
K1_HD uint32_t k1s_lt_mask(const uint32_t* a, const uint32_t* b) {
  uint32_t u[8];
  return 0u - k1_sub256(u, a, b);
}

// ---- GF(p) additions to fe_secp256k1.h ----------------------------------------------------------
// r = 21 a
K1_HD void fe_mul21(K1Fe& r, const K1Fe& a) {
  uint32_t t[8];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)a.v[i] * 21u;
    t[i] = (uint32_t)c;
    c >>= 32;
  }
#pragma unroll
  for (int round = 0; round < 2; round++) {
    // += top (2^32 + 977); top < 21, then the carry out (0 / 1), which cannot carry again
    const uint32_t top = (uint32_t)c;
    c = (uint64_t)t[0] + 977u * top;
    t[0] = (uint32_t)c;
    c >>= 32;
    c += (uint64_t)t[1] + top;
    t[1] = (uint32_t)c;
    c >>= 32;
#pragma unroll
    for (int i = 2; i < 8; i++) {
      c += t[i];
      t[i] = (uint32_t)c;
      c >>= 32;
    }
  }
  fe_final(r, t, 0);
}
K1_HD void fe_sqrn(K1Fe& r, const K1Fe& a, int n) {
  r = a;
#pragma unroll 1
  for (int i = 0; i < n; i++) fe_sqr(r, r);
}
// r = a^(p - 2) = a^-1 (0 -> 0): a fixed chain over the runs of ones of p - 2 = 1^223 0 1^22 0000 1 0 11 0 1,
// 255 squarings and 15 products whatever a is.
K1_HD void fe_inv_ct(K1Fe& r, const K1Fe& a) {
  K1Fe x2, x3, x22, x44, t, u;
  fe_sqr(t, a);
  fe_mul(x2, t, a);
  fe_sqr(t, x2);
  fe_mul(x3, t, a);
  fe_sqrn(t, x3, 3);
  fe_mul(t, t, x3);  // x6
  fe_sqrn(t, t, 3);
  fe_mul(t, t, x3);  // x9
  fe_sqrn(t, t, 2);
  fe_mul(u, t, x2);  // x11
  fe_sqrn(t, u, 11);
  fe_mul(x22, t, u);
  fe_sqrn(t, x22, 22);
  fe_mul(x44, t, x22);
  fe_sqrn(t, x44, 44);
  fe_mul(u, t, x44);  // x88
  fe_sqrn(t, u, 88);
  fe_mul(t, t, u);  // x176
  fe_sqrn(t, t, 44);
  fe_mul(t, t, x44);  // x220
  fe_sqrn(t, t, 3);
  fe_mul(t, t, x3);  // x223
  fe_sqrn(t, t, 23);
  fe_mul(t, t, x22);
  fe_sqrn(t, t, 5);
  fe_mul(t, t, a);
  fe_sqrn(t, t, 3);
  fe_mul(t, t, x2);
  fe_sqrn(t, t, 2);
  fe_mul(r, t, a);
}

// ---- arithmetic mod n additions to sc_secp256k1.h -----------------------------------------------
#define K1_N0INV 0x5588B13Fu  // -n^-1 mod 2^32
// 2^512 mod n
#define K1_NR2_LIMBS \
  { 0x67D7D140u, 0x896CF214u, 0x0E7CF878u, 0x741496C2u, 0x5BCD07C6u, 0xE697F5E4u, 0x81C69BC5u, 0x9D671CD5u }

// r = a b 2^-256 mod n (Montgomery, coarsely integrated operand scanning), a, b < n
K1_HD void scm_mul(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  const uint32_t N[8] = K1_N_LIMBS;
  uint32_t t[10];
#pragma unroll
  for (int i = 0; i < 10; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      c += (uint64_t)a[j] * b[i] + t[j];
      t[j] = (uint32_t)c;
      c >>= 32;
    }
    c += t[8];
    t[8] = (uint32_t)c;
    t[9] = (uint32_t)(c >> 32);
    const uint32_t m = t[0] * K1_N0INV;
    c = (uint64_t)m * N[0] + t[0];
    c >>= 32;
#pragma unroll
    for (int j = 1; j < 8; j++) {
      c += (uint64_t)m * N[j] + t[j];
      t[j - 1] = (uint32_t)c;
      c >>= 32;
    }
    c += t[8];
    t[7] = (uint32_t)c;
    t[8] = t[9] + (uint32_t)(c >> 32);
  }
  // t < 2 n in nine words
  uint32_t u[8];
  const uint32_t borrow = k1_sub256(u, t, N);
  const uint32_t take = 0u - (t[8] | (borrow ^ 1u));
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = k1s_pick(take, u[i], t[i]);
}
// r = a^(n - 2) = a^-1 mod n (0 -> 0), a < n: square and multiply over the bits of the PUBLIC
// exponent (the same 255 squarings and 195 products whatever a is), on Montgomery residues.  The
// exponent shifts through eight words at compile-time indices.
K1_HD void sc_inv_ct(K1Sc& r, const K1Sc& a) {
  const uint32_t R2[8] = K1_NR2_LIMBS;
  uint32_t ex[8] = K1_N_LIMBS;
  ex[0] -= 2u;
  uint32_t am[8], acc[8];
  scm_mul(am, a.v, R2);
#pragma unroll
  for (int i = 0; i < 8; i++) acc[i] = am[i];  // bit 255 of n - 2 is set
#pragma unroll 1
  for (int bit = 254; bit >= 0; bit--) {
#pragma unroll
    for (int j = 7; j > 0; j--) ex[j] = (ex[j] << 1) | (ex[j - 1] >> 31);
    ex[0] <<= 1;
    scm_mul(acc, acc, acc);
    if (ex[7] >> 31) scm_mul(acc, acc, am);  // a bit of n - 2: public
  }
  uint32_t one[8];
#pragma unroll
  for (int i = 0; i < 8; i++) one[i] = i == 0 ? 1u : 0u;
  scm_mul(r.v, acc, one);
}
// r = a + b mod n, a, b < n
K1_HD void sc_add_ct(K1Sc& r, const K1Sc& a, const K1Sc& b) {
  const uint32_t N[8] = K1_N_LIMBS;
  uint32_t t[8], u[8];
  const uint32_t carry = k1_add256(t, a.v, b.v);
  const uint32_t borrow = k1_sub256(u, t, N);
  const uint32_t take = 0u - (carry | (borrow ^ 1u));
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = k1s_pick(take, u[i], t[i]);
}
// a < 2^256 -> a mod q for any q above 2^255 (one masked subtraction)
K1_HD void k1s_reduce_once(uint32_t* r, const uint32_t* a, const uint32_t* q) {
  uint32_t u[8];
  const uint32_t take = 0u - (k1_sub256(u, a, q) ^ 1u);
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = k1s_pick(take, u[i], a[i]);
}

// ---- points: homogeneous projective, complete mixed addition ------------------------------------
struct K1Proj {
  K1Fe x, y, z;
};
K1_HD void gp_set_inf(K1Proj& r) {
  fe_zero(r.x);
  fe_one(r.y);
  fe_zero(r.z);
}
// r = p + q for any p (infinity included) and any affine q on the curve: 11 M + 2 (x 21), no case split
K1_HD void gp_madd(K1Proj& r, const K1Proj& p, const K1Fe& qx, const K1Fe& qy) {
  K1Fe t0, t1, t2, t3, t4, x3, y3, z3;
  fe_mul(t0, p.x, qx);
  fe_mul(t1, p.y, qy);
  fe_add(t3, qx, qy);
  fe_add(t4, p.x, p.y);
  fe_mul(t3, t3, t4);
  fe_add(t4, t0, t1);
  fe_sub(t3, t3, t4);
  fe_mul(t4, qy, p.z);
  fe_add(t4, t4, p.y);
  fe_mul(y3, qx, p.z);
  fe_add(y3, y3, p.x);
  fe_add(x3, t0, t0);
  fe_add(t0, x3, t0);
  fe_mul21(t2, p.z);
  fe_add(z3, t1, t2);
  fe_sub(t1, t1, t2);
  fe_mul21(y3, y3);
  fe_mul(x3, t4, y3);
  fe_mul(t2, t3, t1);
  fe_sub(r.x, t2, x3);
  fe_mul(y3, y3, t0);
  fe_mul(t1, t1, z3);
  fe_add(r.y, t1, y3);
  fe_mul(t0, t0, t3);
  fe_mul(z3, z3, t4);
  fe_add(r.z, z3, t0);
}
// r = m ? a : r
K1_HD void gp_cmov(K1Proj& r, const K1Proj& a, uint32_t m) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    r.x.v[i] = k1s_pick(m, a.x.v[i], r.x.v[i]);
    r.y.v[i] = k1s_pick(m, a.y.v[i], r.y.v[i]);
    r.z.v[i] = k1s_pick(m, a.z.v[i], r.z.v[i]);
  }
}

// P = k G for ANY 256-bit k (0 gives infinity).  Every lane reads all 8 entries of every position
// (addresses depend on j and e only) and keeps one under a mask; the sign is applied by a select;
// a zero digit computes a sum and drops it.  65 additions, no doubling.
K1_HD void ecdsas_comb(K1Proj& P, const uint32_t* k, const uint32_t* __restrict__ tbl) {
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
  gp_set_inf(P);
  {
    K1Fe qx, qy;
    const uint32_t* q = tbl + ECDSAS_TOP_WORD;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      qx.v[i] = q[i];
      qy.v[i] = q[8 + i];
    }
    K1Proj S;
    gp_madd(S, P, qx, qy);
    gp_cmov(P, S, k1s_opaque(0u - carry));
  }
#pragma unroll 1
  for (int j = ECDSAS_NPOS - 1; j >= 0; j--) {
    // the digit is the top nibble, which then moves out (limbs stay at compile-time indices)
    const int32_t d = (int32_t)(t[7] >> 28) - 8;  // [-8, 7]
#pragma unroll
    for (int i = 7; i > 0; i--) t[i] = (t[i] << 4) | (t[i - 1] >> 28);
    t[0] <<= 4;
    const uint32_t sgn = (uint32_t)(d >> 31);  // all ones when negative
    const uint32_t mag = ((uint32_t)d ^ sgn) - sgn;  // 0..8
    K1Fe qx, qy;
    fe_zero(qx);
    fe_zero(qy);
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
    K1Fe ny;
    fe_neg(ny, qy);
    const uint32_t neg = k1s_opaque(sgn);
#pragma unroll
    for (int i = 0; i < 8; i++) qy.v[i] = k1s_pick(neg, ny.v[i], qy.v[i]);
    K1Proj S;
    gp_madd(S, P, qx, qy);  // digit 0: Q = (0, 0), the sum is dropped
    gp_cmov(P, S, k1s_opaque(0u - ((mag | (0u - mag)) >> 31)));
  }
}

// Table lane j: the multiples 1..8 of 16^j G (j < 64) or 2^256 G (j = 64), affine.  Public data,
// once per context: the verify path's variable-time point code.
K1_HD void ecdsas_table_lane(uint32_t* tbl, int j) {
  const uint8_t g[64] = ECDSA_G_BYTES;
  K1Aff base;
  (void)fe_from_be(base.x, g);
  (void)fe_from_be(base.y, g + 32);
  K1Jac a;
  ge_from_aff(a, base);
#pragma unroll 1
  for (int i = 0; i < 4 * j; i++) ge_dbl(a, a);
  ge_to_aff(base, a);
  uint32_t* o = j < ECDSAS_NPOS ? tbl + (size_t)j * (ECDSAS_ENTRIES * 16) : tbl + ECDSAS_TOP_WORD;
  const int entries = j < ECDSAS_NPOS ? ECDSAS_ENTRIES : 1;
  ge_from_aff(a, base);
#pragma unroll 1
  for (int e = 1; e <= entries; e++) {
    K1Aff q = base;
    if (e > 1) {
      ge_madd(a, a, base);  // e = 2 is the doubling branch
      ge_to_aff(q, a);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      o[(e - 1) * 16 + i] = q.x.v[i];
      o[(e - 1) * 16 + 8 + i] = q.y.v[i];
    }
  }
}

// ---- HMAC-SHA-256 DRBG of RFC 6979 §3.2 (fixed input lengths: 97, 33 and 32 bytes) ---------------
struct K1Hmac {  // SHA-256 states after the key's inner and outer pad blocks
  uint32_t i[8], o[8];
};
struct K1Drbg {
  K1Hmac hk;
  uint32_t V[8];  // big-endian words
};
K1_HD void k1s_sha_iv(uint32_t* h) {
  const uint32_t h0[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                          0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = h0[i];
}
K1_HD void k1s_hmac_key(K1Hmac& hk, const uint32_t* K) {
  uint32_t blk[16];
#pragma unroll
  for (int j = 0; j < 16; j++) blk[j] = (j < 8 ? K[j] : 0u) ^ 0x36363636u;
  k1s_sha_iv(hk.i);
  ecdsa_sha256_block(hk.i, blk);
#pragma unroll
  for (int j = 0; j < 16; j++) blk[j] = (j < 8 ? K[j] : 0u) ^ 0x5c5c5c5cu;
  k1s_sha_iv(hk.o);
  ecdsa_sha256_block(hk.o, blk);
}
// out = SHA-256(opad block || inner digest)
K1_HD void k1s_hmac_outer(uint32_t* out, const K1Hmac& hk, const uint32_t* inner) {
  uint32_t blk[16], st[8];
#pragma unroll
  for (int j = 0; j < 16; j++) blk[j] = j < 8 ? inner[j] : 0u;
  blk[8] = 0x80000000u;
  blk[15] = (64 + 32) * 8;
#pragma unroll
  for (int j = 0; j < 8; j++) st[j] = hk.o[j];
  ecdsa_sha256_block(st, blk);
#pragma unroll
  for (int j = 0; j < 8; j++) out[j] = st[j];
}
// out = HMAC(V) (sep < 0) or HMAC(V || sep); out may be V
K1_HD void k1s_hmac_v(uint32_t* out, const K1Hmac& hk, const uint32_t* V, int sep) {
  uint32_t blk[16], st[8];
#pragma unroll
  for (int j = 0; j < 16; j++) blk[j] = j < 8 ? V[j] : 0u;
  blk[8] = sep < 0 ? 0x80000000u : (((uint32_t)sep << 24) | 0x00800000u);
  blk[15] = sep < 0 ? (64 + 32) * 8 : (64 + 33) * 8;
#pragma unroll
  for (int j = 0; j < 8; j++) st[j] = hk.i[j];
  ecdsa_sha256_block(st, blk);
  k1s_hmac_outer(out, hk, st);
}
// out = HMAC(V || sep || x || h): 97 bytes, x and h as big-endian words
K1_HD void k1s_hmac_seed(uint32_t* out, const K1Hmac& hk, const uint32_t* V, uint32_t sep, const uint32_t* x,
                         const uint32_t* h) {
  uint32_t blk[16], st[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    st[j] = hk.i[j];
    blk[j] = V[j];
  }
  blk[8] = (sep << 24) | (x[0] >> 8);
#pragma unroll
  for (int j = 1; j < 8; j++) blk[8 + j] = (x[j - 1] << 24) | (x[j] >> 8);
  ecdsa_sha256_block(st, blk);
  blk[0] = (x[7] << 24) | (h[0] >> 8);
#pragma unroll
  for (int j = 1; j < 8; j++) blk[j] = (h[j - 1] << 24) | (h[j] >> 8);
  blk[8] = (h[7] << 24) | 0x00800000u;
#pragma unroll
  for (int j = 9; j < 15; j++) blk[j] = 0u;
  blk[15] = (64 + 97) * 8;
  ecdsa_sha256_block(st, blk);
  k1s_hmac_outer(out, hk, st);
}
// steps b to g: x (limbs, below q), h1 (the digest's big-endian words), q (limbs, above 2^255)
K1_HD void ecdsas_drbg_init(K1Drbg& d, const uint32_t* x, const uint32_t* h1, const uint32_t* q) {
  uint32_t z[8], xb[8], hb[8], K[8];
#pragma unroll
  for (int i = 0; i < 8; i++) z[i] = h1[7 - i];
  k1s_reduce_once(z, z, q);  // bits2octets
#pragma unroll
  for (int i = 0; i < 8; i++) {
    xb[i] = x[7 - i];
    hb[i] = z[7 - i];
    K[i] = 0u;
    d.V[i] = 0x01010101u;
  }
  k1s_hmac_key(d.hk, K);
#pragma unroll 1
  for (uint32_t sep = 0; sep < 2; sep++) {
    k1s_hmac_seed(K, d.hk, d.V, sep, xb, hb);
    k1s_hmac_key(d.hk, K);
    k1s_hmac_v(d.V, d.hk, d.V, -1);
  }
}
// step h: the next candidate (limbs); all ones iff 1 <= k < q
K1_HD uint32_t ecdsas_drbg_candidate(K1Drbg& d, uint32_t* k, const uint32_t* q) {
  k1s_hmac_v(d.V, d.hk, d.V, -1);
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = d.V[7 - i];
  return k1s_nonzero_mask(k) & k1s_lt_mask(k, q);
}
// step h.3: the candidate was refused
K1_HD void ecdsas_drbg_reject(K1Drbg& d) {
  uint32_t K[8];
  k1s_hmac_v(K, d.hk, d.V, 0);
  k1s_hmac_key(d.hk, K);
  k1s_hmac_v(d.V, d.hk, d.V, -1);
}
// The RFC 6979 nonce for the order q after `skip` usable candidates were refused later (r = 0 or
// s = 0, step h.3): candidates are drawn in order, one outside [1, q - 1] is refused, and so are
// the first `skip` ones inside it.  Returns the number of candidates refused.  The DRBG is run from
// its start, so a caller that retries keeps no DRBG state alive across the signature.
K1_HD uint32_t ecdsas_nonce_skip(uint32_t* k, const uint32_t* x, const uint32_t* h1, const uint32_t* q, uint32_t skip) {
  K1Drbg d;
  ecdsas_drbg_init(d, x, h1, q);
  uint32_t refused = 0;
#pragma unroll 1
  for (;;) {
    const uint32_t ok = ecdsas_drbg_candidate(d, k, q);
    if (ok && refused >= skip) break;  // secret-derived: taken again only after a refused candidate
    if (!ok) skip++;                   // an out-of-range candidate does not count towards skip
    ecdsas_drbg_reject(d);
    refused++;
  }
  return refused;
}
// skip = 0: the first candidate in [1, q - 1]
K1_HD uint32_t ecdsas_nonce(uint32_t* k, const uint32_t* x, const uint32_t* h1, const uint32_t* q) {
  return ecdsas_nonce_skip(k, x, h1, q, 0u);
}

// ---- one signature -------------------------------------------------------------------------------
// r, s for the nonce k (1 <= k < n), the key x (< n) and the reduced digest e (< n); all ones
// unless r = 0 or s = 0
K1_HD uint32_t ecdsas_sign_with_k(K1Sc& r, K1Sc& s, const uint32_t* x, const K1Sc& e, const uint32_t* k,
                                  const uint32_t* __restrict__ tbl) {
  K1Proj R;
  ecdsas_comb(R, k, tbl);
  K1Fe zi, xa;
  fe_inv_ct(zi, R.z);
  fe_mul(xa, R.x, zi);
  const uint32_t N[8] = K1_N_LIMBS;
  k1s_reduce_once(r.v, xa.v, N);  // x(R) < p < 2 n
  K1Sc kk, ki, xs, t;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    kk.v[i] = k[i];
    xs.v[i] = x[i];
  }
  sc_inv_ct(ki, kk);
  sc_mul(t, r, xs);
  sc_add_ct(t, t, e);
  sc_mul(s, ki, t);
  return k1s_nonzero_mask(r.v) & k1s_nonzero_mask(s.v);
}
// sig[0..16): r || s as big-endian words in memory order (sig[i] holds bytes 4 i .. 4 i + 3)
K1_HD void ecdsas_put_sig(uint32_t* sig, const K1Sc& r, const K1Sc& s) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    sig[i] = __builtin_bswap32(r.v[7 - i]);
    sig[8 + i] = __builtin_bswap32(s.v[7 - i]);
  }
}
// One signature under a usable key x (1 <= x < n): h1 = the digest's big-endian words
K1_HD void ecdsas_sign_lane(uint32_t* sig, const uint32_t* x, const uint32_t* h1, const uint32_t* __restrict__ tbl) {
  const uint32_t N[8] = K1_N_LIMBS;
  uint32_t z[8];
#pragma unroll
  for (int i = 0; i < 8; i++) z[i] = h1[7 - i];
  K1Sc e, r, s;
  sc_reduce256(e, z);
#pragma unroll 1
  for (uint32_t skip = 0;; skip++) {
    // r = 0 or s = 0 (probability about 2^-255): the generator is run again from its start and
    // passes over the candidates already refused, so no DRBG state is alive across the signature
    uint32_t k[8];
    (void)ecdsas_nonce_skip(k, x, h1, N, skip);
    if (ecdsas_sign_with_k(r, s, x, e, k, tbl)) break;
  }
  ecdsas_put_sig(sig, r, s);
}

// Signer record from 32 big-endian bytes: x = 0 or x >= n gets a zero record (validity clear).
K1_HD void ecdsas_signer_lane(uint32_t* rec, const uint8_t* priv, const uint32_t* __restrict__ tbl) {
  const uint32_t N[8] = K1_N_LIMBS;
  uint32_t x[8];
  k1_from_be(x, priv);
  const uint32_t ok = k1s_opaque(k1s_nonzero_mask(x) & k1s_lt_mask(x, N));
#pragma unroll
  for (int i = 0; i < 8; i++) x[i] &= ok;
  K1Proj Q;
  ecdsas_comb(Q, x, tbl);  // x = 0: infinity, Z = 0, whose "inverse" is 0: Q = (0, 0)
  K1Fe zi, qx, qy;
  fe_inv_ct(zi, Q.z);
  fe_mul(qx, Q.x, zi);
  fe_mul(qy, Q.y, zi);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    rec[i] = x[i];
    rec[8 + i] = qx.v[i] & ok;
    rec[16 + i] = qy.v[i] & ok;
    rec[24 + i] = i == 0 ? (ok & 1u) : 0u;
  }
}

#if defined(__HIPCC__)
// One batch of messages to sign, all pointers in device memory.
struct EcdsaSignBatch {
  size_t n;
  const uint32_t* signers;     // nkeys x ECDSAS_WORDS
  uint32_t nkeys;
  const uint32_t* signer_idx;  // nullable: every message is signed by signer 0
  const uint8_t* msg;          // message blob
  const uint64_t* msg_off;     // n byte offsets into msg; nullptr = fixed-length messages
  const uint32_t* msg_len;     // n lengths (unused when msg_off is nullptr)
  uint32_t fixed_len;          // msg_off == nullptr: message i = msg[i * fixed_len, (i + 1) * fixed_len)
};
hipError_t cbft_ecdsa_sign_build_table(uint32_t* d_tbl, hipStream_t stream);
// private keys (nkeys x 32 B big-endian, device) -> signer records
hipError_t cbft_ecdsa_sign_launch_keys(const uint8_t* d_priv, uint32_t nkeys, const uint32_t* d_tbl,
                                       uint32_t* d_signers, hipStream_t stream);
// words of per-batch scratch: k[8][n] (secret while it lives: the point kernel zeroes it) | h1[8][n] | state[n]
inline size_t cbft_ecdsa_sign_scratch_words(size_t n) { return 17 * n; }
// d_sig: n x 64 B (4-byte aligned); a signer index >= nkeys or an unusable signer gives 64 zero bytes
hipError_t cbft_ecdsa_sign_launch(const EcdsaSignBatch& b, const uint32_t* d_tbl, uint32_t* d_scratch, uint8_t* d_sig,
                                  hipStream_t stream);
#endif
