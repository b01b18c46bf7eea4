// Batched RSA-2048 PKCS#1 v1.5 / SHA-256 signing with the CRT: launch interface of
// rsa_sign.hip and the constant-time device helpers it is built from (also compiled into
// tests/hip/rsa_sign_selftest.hip).
//
// Reference behaviour: concord::util::crypto::RSASigner::sign = Crypto++ RSASS<PKCS1v15, SHA256>::
// Signer::SignMessage, byte for byte OpenSSL 3.0.2 EVP_DigestSign (RSA, SHA-256); restated in
// oracle/rsa_ref.py:sign.
//
// Secret independence.  p, q, dP, dQ, qInv, m_p, m_q, h and every intermediate enter arithmetic
// and masked selects only: no branch, loop bound, memory address or choice of load depends on
// them.  The message, its length, the signer index, e and n are public.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define RSAS_NL 37                // 28-bit limbs of a value < R' = 2^1036
#define RSAS_PRIV_BYTES 640       // p | q | dP | dQ | qInv, 128 B big-endian each
#define RSAS_WIN 4                // fixed exponent window
#define RSAS_TBL (1 << RSAS_WIN)  // table entries x^0 .. x^15 per lane
#define RSAS_PSIG 32              // signatures per 64-lane block (even lane mod p, odd lane mod q)
// Signer record (uint32 words).  Two halves of RSAS_HALF words, half 0 for p and half 1 for q:
//   modulus m [37] | R'^2 mod m [37] | R' mod m [37] | CRT exponent (32 words, little-endian) |
//   -m^-1 mod 2^28 | pad
// then qInv * R' mod p [37] | e | status | structural checks | pad.  n = p q lives in the verify
// record that is built beside each signer record (rsa_verify.h) and runs the fault check.
#define RSAS_HALF 144
#define RSAS_M 0
#define RSAS_R2 37
#define RSAS_ONE 74
#define RSAS_D 111
#define RSAS_N0INV 143
#define RSAS_QINV 288
#define RSAS_E 325
#define RSAS_STATUS 326
#define RSAS_STRUCT 327
#define RSAS_WORDS 328

// One batch of messages to sign, all pointers in device memory.
struct RsaSignBatch {
  size_t n;
  const uint32_t* signers;     // nkeys x RSAS_WORDS
  uint32_t nkeys;
  const uint32_t* signer_idx;  // nullable: every message is signed by signer 0
  const uint8_t* msg;
  const uint64_t* msg_off;     // nullptr = fixed-length messages
  const uint32_t* msg_len;
  uint32_t fixed_len;
};

// signatures one launch takes (the window tables of a launch are n x 4,736 B of scratch)
#define RSAS_MAX_LAUNCH 65536
// words of per-batch scratch: the window tables ([block][entry][limb][lane]); secret while a batch runs,
// zeroed by the signing kernel before it ends
size_t cbft_rsa_sign_scratch_words(size_t n);
// priv (nkeys x 640 B, device) -> signer records (status word still 0) and the moduli n = p q
// (nkeys x 256 B big-endian, device)
hipError_t cbft_rsa_sign_launch_keys(const uint8_t* d_priv, const uint32_t* d_exp, uint32_t nkeys,
                                     uint32_t* d_signers, uint8_t* d_mod, hipStream_t stream);
// d_sig: n x 256 B (4-byte aligned), no fault check applied yet
hipError_t cbft_rsa_sign_launch(const RsaSignBatch& b, uint32_t* d_scratch, uint8_t* d_sig, hipStream_t stream);
// The verify kernel's inputs for the fault check: idx[i] (0 for an index out of range), off, len
hipError_t cbft_rsa_sign_launch_prep(const RsaSignBatch& b, uint32_t* d_idx, uint64_t* d_off, uint32_t* d_len,
                                     hipStream_t stream);
// Release gate: signature i leaves only if its verdict bit is set, its signer index is in range
// and (use_status) its signer's status word is 1; otherwise it becomes 256 zero bytes.  In-range
// items zeroed are added to *d_failed (nullable).
hipError_t cbft_rsa_sign_launch_gate(const RsaSignBatch& b, const uint64_t* d_verdicts, int use_status,
                                     uint8_t* d_sig, uint32_t* d_failed, hipStream_t stream);
// Load-time self-test result into the records: status[k] = structural checks && verdict bit k
hipError_t cbft_rsa_sign_launch_status(uint32_t* d_signers, uint32_t nkeys, const uint64_t* d_verdicts,
                                       hipStream_t stream);

// The device helpers: for translation units that hold kernels (they define
// CBFT_RSA_SIGN_DEVICE_HELPERS before including this file).
#ifdef CBFT_RSA_SIGN_DEVICE_HELPERS
#include "sha256.h"

#define RS_INLINE __device__ __forceinline__
constexpr int RS_NL = RSAS_NL;
constexpr uint32_t RS_M28 = (1u << 28) - 1;

// all-ones / zero masks pass through an empty asm statement before use, so that the compiler has
// nothing to turn into a branch (as sign_opaque in ed25519_sign.h)
RS_INLINE uint32_t rs_opaque(uint32_t m) {
  asm volatile("" : "+v"(m));
  return m;
}
RS_INLINE uint32_t rs_pick(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }  // m ? a : b
RS_INLINE uint64_t rs_madc(uint32_t a, uint32_t b, uint64_t c) { return (uint64_t)a * b + c; }

RS_INLINE uint32_t rs_from_odd(uint32_t v) {  // lane 2k <- lane 2k+1 (odd lanes keep their own)
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xF5, 0xF, 0xF, false);  // quad_perm [1,1,3,3]
}
RS_INLINE uint32_t rs_from_even(uint32_t v) {  // lane 2k+1 <- lane 2k
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xA0, 0xF, 0xF, false);  // quad_perm [0,0,2,2]
}

// a = a * x / R' mod m, lazy: for normalised operands (limbs < 2^28) with a * x < R' * m the
// result is < 2m, limbs normalised.  R' = 2^1036 > 2^12 m, so every operand below 64m qualifies.
// Row i adds a_i * x and mu_i * m into columns i .. i + 36, one v_mad_u64_u32 each with no carry
// in between: a column takes at most 37 + 37 products of < 2^56 and one carry of < 2^36, below
// 2^63.  All 37 rows are unrolled, so the columns are registers with fixed names and no shift.
template <int I>
RS_INLINE void rs_mm_rows(uint64_t (&A)[2 * RS_NL], const uint32_t (&a)[RS_NL], const uint32_t (&x)[RS_NL],
                          const uint32_t (&m)[RS_NL], uint32_t n0inv) {
  // rows unroll by template recursion: the unroll pragma gives up on 37 x 74 products
  if constexpr (I < RS_NL) {
#pragma unroll
    for (int c = 0; c < RS_NL; c++) A[I + c] = rs_madc(a[I], x[c], A[I + c]);
    const uint32_t mu = ((uint32_t)A[I] * n0inv) & RS_M28;
#pragma unroll
    for (int c = 0; c < RS_NL; c++) A[I + c] = rs_madc(mu, m[c], A[I + c]);
    A[I + 1] += A[I] >> 28;
    rs_mm_rows<I + 1>(A, a, x, m, n0inv);
  }
}
RS_INLINE void rs_mm(uint32_t (&a)[RS_NL], const uint32_t (&x)[RS_NL], const uint32_t (&m)[RS_NL], uint32_t n0inv) {
  uint64_t A[2 * RS_NL];
#pragma unroll
  for (int c = 0; c < 2 * RS_NL; c++) A[c] = 0;
  rs_mm_rows<0>(A, a, x, m, n0inv);
  uint64_t cy = 0;
#pragma unroll
  for (int c = 0; c < RS_NL; c++) {
    cy += A[RS_NL + c];
    a[c] = (uint32_t)cy & RS_M28;
    cy >>= 28;
  }
}

// a = a - m if a >= m (a < 2m): masked select, no loads behind it
RS_INLINE void rs_csub(uint32_t (&a)[RS_NL], const uint32_t (&m)[RS_NL]) {
  uint32_t d[RS_NL];
  int32_t br = 0;
#pragma unroll
  for (int c = 0; c < RS_NL; c++) {
    const int32_t v = (int32_t)a[c] - (int32_t)m[c] + br;
    d[c] = (uint32_t)v & RS_M28;
    br = v >> 28;  // 0 or -1
  }
  const uint32_t keep = rs_opaque((uint32_t)br);  // all ones: a < m
#pragma unroll
  for (int c = 0; c < RS_NL; c++) a[c] = rs_pick(keep, a[c], d[c]);
}

// a = a + b, carries resolved (the sum must stay below 2^1036)
RS_INLINE void rs_add(uint32_t (&a)[RS_NL], const uint32_t (&b)[RS_NL]) {
  uint32_t cy = 0;
#pragma unroll
  for (int c = 0; c < RS_NL; c++) {
    const uint32_t v = a[c] + b[c] + cy;
    a[c] = v & RS_M28;
    cy = v >> 28;
  }
}

// a = b + 2m - a for b < m and a < 2m: in (0, 3m), never negative, so no sign to select on
RS_INLINE void rs_rsub2m(uint32_t (&a)[RS_NL], const uint32_t (&b)[RS_NL], const uint32_t (&m)[RS_NL]) {
  int32_t cy = 0;
#pragma unroll
  for (int c = 0; c < RS_NL; c++) {
    const int32_t v = (int32_t)b[c] + 2 * (int32_t)m[c] - (int32_t)a[c] + cy;
    a[c] = (uint32_t)v & RS_M28;
    cy = v >> 28;
  }
}

// 28-bit limb i of a number given as NW 32-bit little-endian words
template <int NW>
RS_INLINE uint32_t rs_limb28(const uint32_t (&w)[NW], int i) {
  const int o = 28 * i, k = o >> 5, sh = o & 31;
  const uint64_t lo = k < NW ? w[k] : 0u, hi = k + 1 < NW ? w[k + 1] : 0u;
  return (uint32_t)(((hi << 32) | lo) >> sh) & RS_M28;
}

template <int I>
RS_INLINE void rs_mul_rows(uint64_t (&A)[2 * RS_NL], const uint32_t (&a)[RS_NL], const uint32_t (&b)[RS_NL]) {
  if constexpr (I < RS_NL) {
#pragma unroll
    for (int c = 0; c < RS_NL; c++) A[I + c] = rs_madc(a[I], b[c], A[I + c]);
    rs_mul_rows<I + 1>(A, a, b);
  }
}
// out (64 little-endian 32-bit words) = add + a * b for 37-limb a, b, add (the value is < 2^2048)
RS_INLINE void rs_mul_add(uint32_t (&out)[64], const uint32_t (&a)[RS_NL], const uint32_t (&b)[RS_NL],
                          const uint32_t (&add)[RS_NL]) {
  uint64_t A[2 * RS_NL];
#pragma unroll
  for (int c = 0; c < 2 * RS_NL; c++) A[c] = c < RS_NL ? add[c] : 0u;
  rs_mul_rows<0>(A, a, b);
  uint32_t l[2 * RS_NL + 1];
  uint64_t cy = 0;
#pragma unroll
  for (int c = 0; c < 2 * RS_NL; c++) {
    cy += A[c];
    l[c] = (uint32_t)cy & RS_M28;
    cy >>= 28;
  }
  l[2 * RS_NL] = 0;
#pragma unroll
  for (int k = 0; k < 64; k++) {
    const int o = 32 * k, i = o / 28, sh = o % 28;
    const uint64_t v = (uint64_t)l[i] | ((uint64_t)l[i + 1] << 28);
    out[k] = (uint32_t)(v >> sh);
  }
}

// The window tables of one 64-lane block in the batch scratch: tl is the block's part plus the
// lane number, entry e, limb c of the lane is tl[(e * 37 + c) * 64].  Addresses depend on e, c
// and the lane number alone.
RS_INLINE void rs_tbl_store(uint32_t* tl, int e, const uint32_t (&v)[RS_NL]) {
#pragma unroll
  for (int c = 0; c < RS_NL; c++) tl[(e * RS_NL + c) * 64] = v[c];
}
RS_INLINE void rs_tbl_load(uint32_t (&v)[RS_NL], const uint32_t* tl, int e) {
#pragma unroll
  for (int c = 0; c < RS_NL; c++) v[c] = tl[(e * RS_NL + c) * 64];
}
// t = entry `digit`: every entry is read, one is kept by an opaque mask
RS_INLINE void rs_tbl_scan(uint32_t (&t)[RS_NL], const uint32_t* tl, uint32_t digit) {
#pragma unroll
  for (int c = 0; c < RS_NL; c++) t[c] = 0;
#pragma unroll 1
  for (int e = 0; e < RSAS_TBL; e++) {
    // digit ^ e is 0 on a hit and 1..15 otherwise: minus one is negative on a hit alone
    const uint32_t hit = rs_opaque((uint32_t)((int32_t)((digit ^ (uint32_t)e) - 1u) >> 31));
#pragma unroll
    for (int c = 0; c < RS_NL; c++) t[c] = rs_pick(hit, tl[(e * RS_NL + c) * 64], t[c]);
  }
}

// The CRT core of one lane pair: s = EM^d mod n from the record's CRT parameters, as 64
// little-endian words (meaningful in the even lane).  em74: the 74 28-bit limbs of EM (public).
// tl: the lane's window table in the scratch (zeroed again before return).  `hi`: odd lane.
//
// Every step is x = x * y / R' mod m with y chosen by the step number alone:
//   0..2     into Montgomery form: EM = H * R' + Lo; Lo -> Lo R', H -> H R' -> H R'^2; x = their sum
//   3..16    table x^2 .. x^15 (entries 0 and 1 are R' mod m and x)
//   17..1296 256 windows, top first: four squarings, one multiply by the scanned entry (zero
//            windows multiply by entry 0 = one; the top window starts from one like the others)
//   1297     out of Montgomery form and fully reduced: m_p (even lane), m_q (odd lane)
//   1298     even lane: u = m_q mod p as m_q * (R' mod p) / R'; then d = m_p + 2p - u > 0
//   1299     even lane: h = d * (qInv R') / R' mod p, fully reduced
// and s = m_q + h q.  The odd lane runs steps 1298 and 1299 on its own values; nothing is kept.
RS_INLINE void rs_crt_core(uint32_t (&s)[64], const uint32_t* rec, bool hi, const uint32_t (&em74)[2 * RS_NL],
                           uint32_t* tl) {
  const uint32_t* hrec = rec + (hi ? RSAS_HALF : 0);
  uint32_t m[RS_NL], x[RS_NL], y[RS_NL];
#pragma unroll
  for (int c = 0; c < RS_NL; c++) m[c] = hrec[RSAS_M + c];
  const uint32_t n0inv = hrec[RSAS_N0INV];
  // EM's limbs wait in entries 3 (Lo) and 4 (H) until steps 0 and 1 take them
#pragma unroll
  for (int c = 0; c < RS_NL; c++) {
    tl[(3 * RS_NL + c) * 64] = em74[c];
    tl[(4 * RS_NL + c) * 64] = em74[RS_NL + c];
    x[c] = 0;
  }
  constexpr int S_TBL = 3, S_EXP = 17, S_OUT = S_EXP + 5 * (1024 / RSAS_WIN), S_END = S_OUT + 3;
#pragma unroll 1
  for (int step = 0; step < S_END; step++) {
    // the modulus limbs are opaque to loop-invariant code motion (their zero-extended 64-bit
    // copies would be hoisted out of the loop otherwise, as in the verify kernel)
#pragma unroll
    for (int c = 0; c < RS_NL; c++) asm volatile("" : "+v"(m[c]));
    // and so is the table pointer: the 592 addresses behind it are formed where they are used,
    // not kept in registers across the loop
    asm volatile("" : "+v"(tl));
    if (step < S_TBL) {
      if (step == 0) rs_tbl_load(x, tl, 3);
      if (step == 1) rs_tbl_load(x, tl, 4);
#pragma unroll
      for (int c = 0; c < RS_NL; c++) y[c] = hrec[RSAS_R2 + c];
    } else if (step < S_EXP) {
      rs_tbl_load(y, tl, 1);
    } else if (step < S_OUT) {
      const int k = step - S_EXP, w = 1024 / RSAS_WIN - 1 - k / 5;
      if (k % 5 == 4) {
        const uint32_t digit = (hrec[RSAS_D + (w >> 3)] >> (4 * (w & 7))) & 15u;
        rs_tbl_scan(y, tl, digit);
      } else {
#pragma unroll
        for (int c = 0; c < RS_NL; c++) y[c] = x[c];
      }
    } else if (step == S_OUT) {
#pragma unroll
      for (int c = 0; c < RS_NL; c++) y[c] = c == 0 ? 1u : 0u;
    } else if (step == S_OUT + 1) {
#pragma unroll
      for (int c = 0; c < RS_NL; c++) y[c] = hrec[RSAS_ONE + c];
    } else {
#pragma unroll
      for (int c = 0; c < RS_NL; c++) y[c] = rec[RSAS_QINV + c];
    }

    rs_mm(x, y, m, n0inv);

    if (step == 0) {
      rs_tbl_store(tl, 1, x);
    } else if (step == 2) {
      rs_tbl_load(y, tl, 1);
      rs_add(x, y);  // < 4m
      rs_tbl_store(tl, 1, x);
#pragma unroll
      for (int c = 0; c < RS_NL; c++) tl[c * 64] = hrec[RSAS_ONE + c];
    } else if (step >= S_TBL && step < S_EXP) {
      rs_tbl_store(tl, step - 1, x);
      if (step == S_EXP - 1) {
#pragma unroll
        for (int c = 0; c < RS_NL; c++) x[c] = hrec[RSAS_ONE + c];
      }
    } else if (step == S_OUT) {
      rs_csub(x, m);  // m_p | m_q in [0, m)
      rs_tbl_store(tl, 2, x);
#pragma unroll
      for (int c = 0; c < RS_NL; c++) x[c] = rs_from_odd(x[c]);  // even lane: m_q
    } else if (step == S_OUT + 1) {
      rs_tbl_load(y, tl, 2);
      rs_rsub2m(x, y, m);
    } else if (step == S_OUT + 2) {
      rs_csub(x, m);  // h in [0, p)
    }
  }
  // even lane: s = m_q + h q
  uint32_t mq[RS_NL];
  rs_tbl_load(mq, tl, 2);
#pragma unroll
  for (int c = 0; c < RS_NL; c++) {
    mq[c] = rs_from_odd(mq[c]);
    m[c] = rs_from_odd(m[c]);
  }
  rs_mul_add(s, x, m, mq);
  // the tables held powers of EM mod p and mod q, m_p and m_q: none stay behind
#pragma unroll 1
  for (int e = 0; e < RSAS_TBL; e++)
#pragma unroll
    for (int c = 0; c < RS_NL; c++) tl[(e * RS_NL + c) * 64] = 0u;
}

// ---- record build (one lane per key) ----
RS_INLINE uint32_t rs_load_be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}
// x = 2x mod m for x < m < 2^1024, m's top bit set
RS_INLINE void rs_mod_double(uint32_t (&x)[32], const uint32_t (&m)[32]) {
  const uint32_t top = x[31] >> 31;
#pragma unroll
  for (int i = 31; i > 0; i--) x[i] = (x[i] << 1) | (x[i - 1] >> 31);
  x[0] <<= 1;
  uint32_t d[32];
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    const uint64_t v = (uint64_t)x[i] - m[i] - br;
    d[i] = (uint32_t)v;
    br = (uint32_t)(v >> 63);
  }
  const uint32_t ge = rs_opaque(0u - (top | (br ^ 1u)));  // all ones: 2x >= m
#pragma unroll
  for (int i = 0; i < 32; i++) x[i] = rs_pick(ge, d[i], x[i]);
}

// One half of a record from the 1,024-bit modulus md and CRT exponent ex (big-endian bytes):
// limbs, -m^-1 mod 2^28, R'^2 mod m by 1,048 modular doublings of 2^1024 - m, the exponent words.
// Returns 1 if m is odd and exactly 1,024 bits.  R' mod m is filled in by the caller.
RS_INLINE uint32_t rs_build_half(uint32_t* hrec, const uint8_t* md, const uint8_t* ex) {
  uint32_t m[32], x[32];
#pragma unroll
  for (int i = 0; i < 32; i++) m[i] = rs_load_be32(md + 128 - 4 * (i + 1));
  uint32_t inv = m[0];
  for (int it = 0; it < 4; it++) inv *= 2u - m[0] * inv;
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    const uint64_t d = 0ull - m[i] - br;
    x[i] = (uint32_t)d;
    br = (uint32_t)(d >> 63);
  }
#pragma unroll 1
  for (int it = 0; it < 2 * 28 * RS_NL - 1024; it++) rs_mod_double(x, m);
#pragma unroll
  for (int c = 0; c < RS_NL; c++) {
    hrec[RSAS_M + c] = rs_limb28<32>(m, c);
    hrec[RSAS_R2 + c] = rs_limb28<32>(x, c);
  }
#pragma unroll
  for (int i = 0; i < 32; i++) hrec[RSAS_D + i] = rs_load_be32(ex + 128 - 4 * (i + 1));
  hrec[RSAS_N0INV] = (0u - inv) & RS_M28;
  return (m[0] & 1u) & (m[31] >> 31);
}

// The whole record of one key (status word left 0) and its modulus n = p q, big-endian.
RS_INLINE void rs_build_record(uint32_t* rec, const uint8_t* priv, uint32_t e, uint8_t* mod_out) {
  uint32_t ok = rs_build_half(rec, priv, priv + 256);
  ok &= rs_build_half(rec + RSAS_HALF, priv + 128, priv + 384);
  uint32_t qi[32];
#pragma unroll
  for (int i = 0; i < 32; i++) qi[i] = rs_load_be32(priv + 512 + 128 - 4 * (i + 1));
  // products, chosen by the step number: R' mod p, R' mod q, qInv R' mod p, q mod p, q qInv mod p
  uint32_t m[RS_NL], x[RS_NL], y[RS_NL];
#pragma unroll
  for (int c = 0; c < RS_NL; c++) x[c] = 0;
#pragma unroll 1
  for (int step = 0; step < 5; step++) {
    uint32_t* hrec = rec + (step == 1 ? RSAS_HALF : 0);
#pragma unroll
    for (int c = 0; c < RS_NL; c++) {
      m[c] = hrec[RSAS_M + c];
      if (step < 2) x[c] = hrec[RSAS_R2 + c], y[c] = c == 0 ? 1u : 0u;
      if (step == 2) x[c] = rs_limb28<32>(qi, c), y[c] = rec[RSAS_R2 + c];
      if (step == 3) x[c] = rec[RSAS_HALF + RSAS_M + c], y[c] = rec[RSAS_ONE + c];
      if (step == 4) y[c] = rec[RSAS_QINV + c];
    }
    rs_mm(x, y, m, hrec[RSAS_N0INV]);
    if (step < 2) {
#pragma unroll
      for (int c = 0; c < RS_NL; c++) hrec[RSAS_ONE + c] = x[c];
    }
    if (step == 2) {
#pragma unroll
      for (int c = 0; c < RS_NL; c++) rec[RSAS_QINV + c] = x[c];
    }
  }
  rs_csub(x, m);  // q qInv mod p, fully reduced: must be 1
  uint32_t diff = x[0] ^ 1u, same = 0;
#pragma unroll
  for (int c = 1; c < RS_NL; c++) diff |= x[c];
  // n = p q (m holds p's limbs), p != q
  uint32_t nw[64], zero[RS_NL];
#pragma unroll
  for (int c = 0; c < RS_NL; c++) {
    y[c] = rec[RSAS_HALF + RSAS_M + c];
    zero[c] = 0;
    same |= y[c] ^ m[c];
  }
  rs_mul_add(nw, m, y, zero);
  ok &= (nw[63] >> 31) & (uint32_t)(diff == 0) & (uint32_t)(same != 0);
#pragma unroll
  for (int k = 0; k < 64; k++) {
    const uint32_t v = nw[63 - k];
    mod_out[4 * k] = (uint8_t)(v >> 24), mod_out[4 * k + 1] = (uint8_t)(v >> 16);
    mod_out[4 * k + 2] = (uint8_t)(v >> 8), mod_out[4 * k + 3] = (uint8_t)v;
  }
  rec[RSAS_E] = e;
  rec[RSAS_STATUS] = 0;
  rec[RSAS_STRUCT] = ok;
}
#endif  // CBFT_RSA_SIGN_DEVICE_HELPERS
