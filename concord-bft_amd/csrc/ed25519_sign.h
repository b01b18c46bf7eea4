// Batched Ed25519 signing (RFC 8032 §5.1.6): launch interface of ed25519_sign.hip and the
// constant-time device helpers it is built from (also compiled into tests/hip/sign_selftest.hip).
//
// Secret independence.  a, prefix, r and every intermediate of [r]B and [a]B enter arithmetic and
// selects only: no branch, loop bound, memory address or choice of load depends on them.  The
// verify kernels' helpers that break this rule (ge_add_mem's sign-indexed load, the digit-indexed
// comb ladders, fe_invert_var / safegcd) are not used here; see DESIGN.md §14.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// Fixed-base comb of B in signed radix 16: position j (0..63) holds e * 16^j * B, e = 1..8, as
// affine Niels points (y+x, y-x, 2dxy; 9 limbs each, one pad word).  64 x 8 x 28 words = 56 KiB.
#define CBFT_SIGN_W 4
#define CBFT_SIGN_NPOS 64
#define CBFT_SIGN_ENTRIES 8
#define CBFT_SIGN_NIELS_WORDS 28
#define CBFT_SIGN_TABLE_WORDS (CBFT_SIGN_NPOS * CBFT_SIGN_ENTRIES * CBFT_SIGN_NIELS_WORDS)
#define CBFT_SIGN_BLOCK 256
// Per-signer record: a (clamped scalar, 8 words) | prefix (8 words) | A = encode([a]B) (8 words)
#define CBFT_SIGNER_WORDS 24

// One batch of messages to sign, all pointers in device memory.
struct Ed25519SignBatch {
  size_t n;
  const uint32_t* signers;     // nkeys x CBFT_SIGNER_WORDS
  uint32_t nkeys;
  const uint32_t* signer_idx;  // nullable: every message is signed by signer 0
  const uint8_t* msg;          // message blob
  const uint64_t* msg_off;     // n byte offsets into msg; nullptr = fixed-length messages
  const uint32_t* msg_len;     // n lengths (unused when msg_off is nullptr)
  uint32_t fixed_len;          // msg_off == nullptr: message i = msg[i * fixed_len, (i + 1) * fixed_len)
};

// words of per-batch scratch (the nonces r, structure of arrays): secret while it lives
inline size_t cbft_ed25519_sign_scratch_words(size_t n) { return 8 * n; }
hipError_t cbft_ed25519_sign_build_table(uint32_t* d_tbl, hipStream_t stream);
// seeds (nkeys x 32 B, device) -> signer records
hipError_t cbft_ed25519_sign_launch_keys(const uint8_t* d_seed, uint32_t nkeys, const uint32_t* d_tbl,
                                         uint32_t* d_signers, hipStream_t stream);
// d_sig: n x 64 B (4-byte aligned); a signer index >= nkeys gives 64 zero bytes
hipError_t cbft_ed25519_sign_launch(const Ed25519SignBatch& b, const uint32_t* d_tbl, uint32_t* d_scratch,
                                    uint8_t* d_sig, hipStream_t stream);

// The device helpers: for translation units that hold kernels (they define CBFT_SIGN_DEVICE_HELPERS
// before including this file); the C ABI sources see the launch interface alone.
#ifdef CBFT_SIGN_DEVICE_HELPERS
#include "ge25519.h"
#include "sc25519.h"
#include "sha512.h"

// p + q for an affine Niels q (Z = 1): the complete extended-coordinates addition, 3M.  No case
// split: q = identity (1, 1, 0) and p = identity (0 : 1 : 1 : 0) go through the same formulas.
FE_INLINE void ge_madd_niels(ge_p1p1& r, const ge_p3& p, const fe& ypx, const fe& ymx, const fe& t2d) {
  fe A, B, C, D, t;
  fe_add(t, p.Y, p.X);    // Lz
  fe_mul(A, t, ypx);
  fe_sub(t, p.Y, p.X);    // R
  fe_mul(B, t, ymx);
  fe_mul(C, t2d, p.T);
  fe_add(D, p.Z, p.Z);    // Lz
  fe_sub(r.X, A, B);      // R
  fe_add(r.Y, A, B);      // Lz
  fe_add(r.Z, D, C);      // 3R -> carry
  fe_carry(r.Z);          // R
  fe_sub(r.T, D, C);      // R
}

// P = sum_j d_j 16^j B for the 64 signed digits held in kp (sc_recode_prepare<4, 64>; popped top
// digit first).  Every lane reads all 8 entries of every position (addresses depend on j and e
// only, the same in every lane of a wave) and keeps one by compare-and-select; the sign is
// applied by selects.  64 additions, no doubling.
//
// The selects are bit masks (all ones / zero) that pass through an empty asm statement before
// use.  Written as `hit ? q[i] : old`, the compiler moved each table load into a block executed
// only when some lane of the wave hits (s_and_saveexec / s_cbranch_execz around an s_load): a
// branch and a load that depend on the digits.  An opaque mask leaves it nothing to branch on:
// every load is issued and every lane runs the same v_bfi_b32 sequence.
FE_INLINE uint32_t sign_opaque(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(m));
#endif
  return m;
}
FE_INLINE uint32_t sign_pick(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }  // m ? a : b

FE_INLINE void sign_comb_mul(ge_p3& P, uint32_t* kp, const uint32_t* __restrict__ tbl) {
  ge_p3_0(P);
#pragma nounroll
  for (int j = CBFT_SIGN_NPOS - 1; j >= 0; j--) {
    const int d = sc_recode_pop<CBFT_SIGN_W>(kp);  // [-8, 7]
    const uint32_t sgn = (uint32_t)(d >> 31);      // all ones when negative
    const uint32_t mag = ((uint32_t)d ^ sgn) - sgn;
    fe ypx, ymx, t2d;  // digit 0: the identity (1, 1, 0)
    fe_1(ypx);
    fe_1(ymx);
    fe_0(t2d);
    const uint32_t* pos = tbl + (size_t)j * (CBFT_SIGN_ENTRIES * CBFT_SIGN_NIELS_WORDS);
#pragma unroll
    for (int e = 1; e <= CBFT_SIGN_ENTRIES; e++) {
      const uint32_t* q = pos + (e - 1) * CBFT_SIGN_NIELS_WORDS;
      // mag ^ e is 0 on a hit and 1..15 otherwise: minus one is negative on a hit alone
      const uint32_t hit = sign_opaque((uint32_t)((int32_t)((mag ^ (uint32_t)e) - 1u) >> 31));
#pragma unroll
      for (int i = 0; i < FE_LIMBS; i++) {
        ypx.v[i] = sign_pick(hit, q[i], ypx.v[i]);
        ymx.v[i] = sign_pick(hit, q[9 + i], ymx.v[i]);
        t2d.v[i] = sign_pick(hit, q[18 + i], t2d.v[i]);
      }
    }
    // -(x, y) = (-x, y): swap y+x <-> y-x, negate 2dxy (as ge_cached_cneg)
    const uint32_t neg = sign_opaque(sgn);
    fe n;
    fe_neg(n, t2d);
#pragma unroll
    for (int i = 0; i < FE_LIMBS; i++) {
      const uint32_t a = ypx.v[i], b = ymx.v[i];
      ypx.v[i] = sign_pick(neg, b, a);
      ymx.v[i] = sign_pick(neg, a, b);
      t2d.v[i] = sign_pick(neg, n.v[i], t2d.v[i]);
    }
    ge_p1p1 t;
    ge_madd_niels(t, P, ypx, ymx, t2d);
    ge_p1p1_to_p3(P, t);
  }
}

// out (8 words) = encode([k]B) for k + 0x88..8 < 2^256 (the recoding's condition): every k < L
// qualifies, a clamped a (up to 2^255) is reduced mod L by the caller first.  Recode, comb,
// constant-time inversion (the Fermat chain fe_invert inside ge_tobytes), encode.
FE_INLINE void sign_base_mul_encode(uint32_t* out, const uint32_t* k8, const uint32_t* __restrict__ tbl) {
  uint32_t kp[9];
  sc_recode_prepare<CBFT_SIGN_W, CBFT_SIGN_NPOS>(kp, k8);
  ge_p3 P;
  sign_comb_mul(P, kp, tbl);
  ge_tobytes(out, P.X, P.Y, P.Z);
}

// Table lane j (0..63): the multiples 1..8 of 16^j B, each normalised to affine Niels form.
// Public data; runs once per context.
FE_INLINE void sign_table_build_lane(uint32_t* tbl, int j) {
  uint32_t bw[8];  // B = (x, 4/5), x even
  bw[0] = 0x66666658u;
  for (int i = 1; i < 8; i++) bw[i] = 0x66666666u;
  ge_p3 Pj, Q;
  ge_frombytes(Pj, bw);
  ge_p1p1 t;
  for (int i = 0; i < CBFT_SIGN_W * j; i++) {
    ge_dbl(t, Pj.X, Pj.Y, Pj.Z);
    ge_p1p1_to_p3(Pj, t);
  }
  ge_cached cP;
  ge_p3_to_cached(cP, Pj);
  Q = Pj;
  fe d2;
  fe_load_const(d2, kFeD2);
  for (int e = 1; e <= CBFT_SIGN_ENTRIES; e++) {
    fe zi, x, y, xy, ypx, ymx, t2d;
    fe_invert(zi, Q.Z);
    fe_mul(x, Q.X, zi);
    fe_mul(y, Q.Y, zi);
    fe_mul(xy, x, y);
    fe_add(ypx, y, x);
    fe_carry(ypx);
    fe_sub(ymx, y, x);
    fe_mul(t2d, xy, d2);
    uint32_t* q = tbl + ((size_t)j * CBFT_SIGN_ENTRIES + (e - 1)) * CBFT_SIGN_NIELS_WORDS;
#pragma unroll
    for (int i = 0; i < FE_LIMBS; i++) {
      q[i] = ypx.v[i];
      q[9 + i] = ymx.v[i];
      q[18 + i] = t2d.v[i];
    }
    q[27] = 0;
    ge_add(t, Q, cP, false);
    ge_p1p1_to_p3(Q, t);
  }
}
#endif  // CBFT_SIGN_DEVICE_HELPERS
