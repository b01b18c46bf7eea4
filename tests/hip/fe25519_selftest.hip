// Test-only device harness (not part of the product library): the Ed25519 lane code of
// csrc/fe25519.h (with the three generated fe25519_asm*.h), sc25519.h and ge25519.h, one function
// per launch on chosen operands, so tests/test_fe25519_lane_gpu.py can compare the COMPILED code on
// gfx950 -- asm statements with their constraint lists and pinned registers included -- with exact
// Python integers at the operand bounds the headers state (tests/fe25519_cases.py).
//
// Layout: one lane per case, (n + 63) / 64 blocks of 64, lanes i >= n return at once.  Lane i reads
// in[i * IN .. ) and writes out[i * OUT .. ), IN and OUT words per operation from st_words() below
// (exported, so the caller sizes its buffers from the same table).  The operation and its variant
// (aliasing form, zIsOne) are template arguments chosen per launch.  Two operations differ:
//   ST_INVERT_VAR_WAVE  one 64-lane block per value, every lane the same input (fe_invert_var<true>
//                       wants the whole wave active on a uniform value), every lane's result returned
//   ST_FROMBYTES_ROW    one 16-lane row per case, the same words in all 16 lanes, every row lane's
//                       result returned; rows past n recompute case n - 1 (as the product's decode
//                       waves clamp) and write nothing
// The device output buffer is filled with ST_SENTINEL bytes before the launch.
#include <hip/hip_runtime.h>

#include "ge25519.h"
#include "sc25519.h"

enum {
  ST_MUL_C = 0,      // fe_mul<true>            a b -> r          variant: 0 r fresh, 1 r is a, 2 r is b, 3 a is b
  ST_MUL_NC,         // fe_mul<false>
  ST_MULF,           // fe_mulf_oneasm
  ST_MUL2,           // fe_mul2_oneasm          a0 b0 a1 b1 -> r0 r1   variant: 0 fresh, 1 r0 is a1 and r1 is b0,
  ST_MULF2,          // fe_mulf2_oneasm                                          2 r0 is a0 and r1 is a1
  ST_SQ_C,           // fe_sq<true>             a -> r            variant: 0 r fresh, 1 r is a
  ST_SQ_NC,          // fe_sq<false>
  ST_MUL_SMALL,      // fe_mul_small            a s -> r          variant: 0 r fresh, 1 r is a
  ST_ADD,            // fe_add                  a b -> r          variant: 0 r fresh, 1 r is a
  ST_SUB,            // fe_sub
  ST_NEG,            // fe_neg                  a -> r            variant: 0 r fresh, 1 r is a
  ST_SUB_LAZY,       // fe_sub_lazy             a b -> r          variant: 0 r fresh, 1 r is a
  ST_CARRY,          // fe_carry                a -> a
  ST_CANON,          // fe_to_words, fe_iszero, fe_isnegative     a -> 8 words, flag, flag
  ST_FROM_WORDS,     // fe_from_words           8 words -> r
  ST_INVERT_C,       // fe_invert<true>         a -> r
  ST_INVERT_NC,      // fe_invert<false>
  ST_INVERT_VAR,     // fe_invert_var<false>
  ST_POW_C,          // fe_pow22523<true>
  ST_POW_NC,         // fe_pow22523<false>
  ST_SC_CANON,       // sc_is_canonical         8 words -> flag
  ST_SC_REDUCE,      // sc_reduce512            16 words -> 8 words
  ST_FROMBYTES,      // ge_frombytes            8 words -> ok X Y T
  ST_GE_DBL,         // ge_dbl, ge_p1p1_to_p3, ge_tobytes         X Y Z -> X Y Z T, 8 words
  ST_GE_ADD,         // ge_p3_to_cached(Q), ge_cached_cneg, ge_add(P, .), ge_p1p1_to_p3, ge_tobytes
                     //                         P Q neg -> X Y Z T, 8 words      variant: zIsOne
  ST_INVERT_VAR_WAVE,  // fe_invert_var<true>   a -> 64 x r
  ST_FROMBYTES_ROW,    // ge_frombytes_row<false>   8 words -> 16 x (ok X Y)
  ST_NOPS
};

#define ST_SENTINEL_BYTE 0xA5
#define F FE_LIMBS

struct StWords {
  int in, out, variants;
};
__host__ __device__ constexpr StWords st_words(int op) {
  switch (op) {
    case ST_MUL_C:
    case ST_MUL_NC:
    case ST_MULF: return {2 * F, F, 4};
    case ST_MUL2:
    case ST_MULF2: return {4 * F, 2 * F, 3};
    case ST_SQ_C:
    case ST_SQ_NC: return {F, F, 2};
    case ST_MUL_SMALL: return {F + 1, F, 2};
    case ST_ADD:
    case ST_SUB:
    case ST_SUB_LAZY: return {2 * F, F, 2};
    case ST_NEG: return {F, F, 2};
    case ST_CARRY: return {F, F, 1};
    case ST_CANON: return {F, 10, 1};
    case ST_FROM_WORDS: return {8, F, 1};
    case ST_INVERT_C:
    case ST_INVERT_NC:
    case ST_INVERT_VAR:
    case ST_POW_C:
    case ST_POW_NC: return {F, F, 1};
    case ST_SC_CANON: return {8, 1, 1};
    case ST_SC_REDUCE: return {16, 8, 1};
    case ST_FROMBYTES: return {8, 1 + 3 * F, 1};
    case ST_GE_DBL: return {3 * F, 4 * F + 8, 1};
    case ST_GE_ADD: return {8 * F + 1, 4 * F + 8, 2};
    case ST_INVERT_VAR_WAVE: return {F, 64 * F, 1};
    case ST_FROMBYTES_ROW: return {8, 16 * (1 + 2 * F), 1};
    default: return {0, 0, 0};
  }
}

FE_INLINE void st_ld(fe& r, const uint32_t* p) {
#pragma unroll
  for (int k = 0; k < F; k++) r.v[k] = p[k];
}
FE_INLINE void st_st(uint32_t* p, const fe& a) {
#pragma unroll
  for (int k = 0; k < F; k++) p[k] = a.v[k];
}

template <int OP>
FE_INLINE void st_mul(fe& r, const fe& a, const fe& b) {
  if (OP == ST_MUL_C) fe_mul<true>(r, a, b);
  if (OP == ST_MUL_NC) fe_mul<false>(r, a, b);
  if (OP == ST_MULF) fe_mulf_oneasm(r, a, b);
}
template <int OP>
FE_INLINE void st_mul2(fe& r0, const fe& a0, const fe& b0, fe& r1, const fe& a1, const fe& b1) {
  if (OP == ST_MUL2) fe_mul2_oneasm(r0, a0, b0, r1, a1, b1);
  if (OP == ST_MULF2) fe_mulf2_oneasm(r0, a0, b0, r1, a1, b1);
}

// one case: x = the lane's IN words, y = its OUT words
template <int OP, int V>
FE_INLINE void st_lane(const uint32_t* x, uint32_t* y) {
  if constexpr (OP == ST_MUL_C || OP == ST_MUL_NC || OP == ST_MULF) {
    fe a, b, r;
    st_ld(a, x);
    st_ld(b, x + F);
    if (V == 0) {
      st_mul<OP>(r, a, b);
      st_st(y, r);
    } else if (V == 1) {
      st_mul<OP>(a, a, b);
      st_st(y, a);
    } else if (V == 2) {
      st_mul<OP>(b, a, b);
      st_st(y, b);
    } else {
      st_mul<OP>(r, a, a);
      st_st(y, r);
    }
  } else if constexpr (OP == ST_MUL2 || OP == ST_MULF2) {
    fe a0, b0, a1, b1, r0, r1;
    st_ld(a0, x);
    st_ld(b0, x + F);
    st_ld(a1, x + 2 * F);
    st_ld(b1, x + 3 * F);
    if (V == 0) {
      st_mul2<OP>(r0, a0, b0, r1, a1, b1);
      st_st(y, r0);
      st_st(y + F, r1);
    } else if (V == 1) {
      st_mul2<OP>(a1, a0, b0, b0, a1, b1);
      st_st(y, a1);
      st_st(y + F, b0);
    } else {
      st_mul2<OP>(a0, a0, b0, a1, a1, b1);
      st_st(y, a0);
      st_st(y + F, a1);
    }
  } else if constexpr (OP == ST_SQ_C || OP == ST_SQ_NC) {
    fe a, r;
    st_ld(a, x);
    if (V == 0) {
      fe_sq<OP == ST_SQ_C>(r, a);
      st_st(y, r);
    } else {
      fe_sq<OP == ST_SQ_C>(a, a);
      st_st(y, a);
    }
  } else if constexpr (OP == ST_MUL_SMALL) {
    fe a, r;
    st_ld(a, x);
    if (V == 0) {
      fe_mul_small(r, a, x[F]);
      st_st(y, r);
    } else {
      fe_mul_small(a, a, x[F]);
      st_st(y, a);
    }
  } else if constexpr (OP == ST_ADD || OP == ST_SUB || OP == ST_SUB_LAZY) {
    fe a, b, r;
    st_ld(a, x);
    st_ld(b, x + F);
    fe& d = V == 0 ? r : a;
    if (OP == ST_ADD) fe_add(d, a, b);
    if (OP == ST_SUB) fe_sub(d, a, b);
    if (OP == ST_SUB_LAZY) fe_sub_lazy(d, a, b);
    st_st(y, d);
  } else if constexpr (OP == ST_NEG) {
    fe a, r;
    st_ld(a, x);
    fe& d = V == 0 ? r : a;
    fe_neg(d, a);
    st_st(y, d);
  } else if constexpr (OP == ST_CARRY) {
    fe a;
    st_ld(a, x);
    fe_carry(a);
    st_st(y, a);
  } else if constexpr (OP == ST_CANON) {
    fe a;
    st_ld(a, x);
    uint32_t w[8];
    fe_to_words(w, a);
#pragma unroll
    for (int k = 0; k < 8; k++) y[k] = w[k];
    y[8] = fe_iszero(a) ? 1u : 0u;
    y[9] = fe_isnegative(a);
  } else if constexpr (OP == ST_FROM_WORDS) {
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = x[k];
    fe r;
    fe_from_words(r, w);
    st_st(y, r);
  } else if constexpr (OP >= ST_INVERT_C && OP <= ST_POW_NC) {
    fe a, r;
    st_ld(a, x);
    if (OP == ST_INVERT_C) fe_invert<true>(r, a);
    if (OP == ST_INVERT_NC) fe_invert<false>(r, a);
    if (OP == ST_INVERT_VAR) fe_invert_var<false>(r, a);
    if (OP == ST_POW_C) fe_pow22523<true>(r, a);
    if (OP == ST_POW_NC) fe_pow22523<false>(r, a);
    st_st(y, r);
  } else if constexpr (OP == ST_SC_CANON) {
    uint32_t s[8];
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = x[k];
    y[0] = sc_is_canonical(s) ? 1u : 0u;
  } else if constexpr (OP == ST_SC_REDUCE) {
    uint32_t s[16], r[8];
#pragma unroll
    for (int k = 0; k < 16; k++) s[k] = x[k];
    sc_reduce512(r, s);
#pragma unroll
    for (int k = 0; k < 8; k++) y[k] = r[k];
  } else if constexpr (OP == ST_FROMBYTES) {
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = x[k];
    ge_p3 h;
    const bool ok = ge_frombytes(h, w);
    y[0] = ok ? 1u : 0u;
    st_st(y + 1, h.X);
    st_st(y + 1 + F, h.Y);
    st_st(y + 1 + 2 * F, h.T);
  } else if constexpr (OP == ST_GE_DBL || OP == ST_GE_ADD) {
    ge_p1p1 t;
    if constexpr (OP == ST_GE_DBL) {
      fe X, Y, Z;
      st_ld(X, x);
      st_ld(Y, x + F);
      st_ld(Z, x + 2 * F);
      ge_dbl(t, X, Y, Z);
    } else {
      ge_p3 P, Q;
      st_ld(P.X, x);
      st_ld(P.Y, x + F);
      st_ld(P.Z, x + 2 * F);
      st_ld(P.T, x + 3 * F);
      st_ld(Q.X, x + 4 * F);
      st_ld(Q.Y, x + 5 * F);
      st_ld(Q.Z, x + 6 * F);
      st_ld(Q.T, x + 7 * F);
      ge_cached c;
      ge_p3_to_cached(c, Q);
      ge_cached_cneg(c, x[8 * F] != 0u);
      ge_add(t, P, c, V != 0);
    }
    ge_p3 R;
    ge_p1p1_to_p3(R, t);
    st_st(y, R.X);
    st_st(y + F, R.Y);
    st_st(y + 2 * F, R.Z);
    st_st(y + 3 * F, R.T);
    uint32_t w[8];
    ge_tobytes(w, R.X, R.Y, R.Z);
#pragma unroll
    for (int k = 0; k < 8; k++) y[4 * F + k] = w[k];
  }
}

template <int OP, int V>
__global__ void __launch_bounds__(64) st_lane_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  st_lane<OP, V>(in + (size_t)i * st_words(OP).in, out + (size_t)i * st_words(OP).out);
}

// one block = one wave = one value; all 64 lanes active on the same input
__global__ void __launch_bounds__(64) st_invert_wave_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                            int n) {
  const int i = blockIdx.x;
  if (i >= n) return;  // (uniform: the grid is n blocks)
  fe a;
  st_ld(a, in + (size_t)i * F);
  fe_invert_var<true>(a, a);
  st_st(out + ((size_t)i * 64 + threadIdx.x) * F, a);
}

// one 16-lane row = one case; whole waves stay active (rows past n recompute case n - 1)
__global__ void __launch_bounds__(64) st_frombytes_row_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                              int n) {
  const int lane = blockIdx.x * 64 + threadIdx.x;
  const int row = lane >> 4;
  const int i = row < n ? row : n - 1;
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = in[(size_t)i * 8 + k];
  fe X, Y;
  const bool ok = ge_frombytes_row<false>(X, Y, w);
  if (row >= n) return;
  uint32_t* y = out + ((size_t)i * 16 + (lane & 15)) * (1 + 2 * F);
  y[0] = ok ? 1u : 0u;
  st_st(y + 1, X);
  st_st(y + 1 + F, Y);
}

template <int OP, int V>
static void st_launch(const uint32_t* d_in, uint32_t* d_out, int n) {
  hipLaunchKernelGGL((st_lane_kernel<OP, V>), dim3((n + 63) / 64), dim3(64), 0, 0, d_in, d_out, n);
}

// false: no such (op, variant)
static bool st_dispatch(int op, int variant, const uint32_t* d_in, uint32_t* d_out, int n) {
#define ST_CASE(OP, V) \
  if (op == OP && variant == V) return st_launch<OP, V>(d_in, d_out, n), true;
#define ST_CASE2(OP) ST_CASE(OP, 0) ST_CASE(OP, 1)
#define ST_CASE3(OP) ST_CASE2(OP) ST_CASE(OP, 2)
#define ST_CASE4(OP) ST_CASE3(OP) ST_CASE(OP, 3)
  ST_CASE4(ST_MUL_C)
  ST_CASE4(ST_MUL_NC)
  ST_CASE4(ST_MULF)
  ST_CASE3(ST_MUL2)
  ST_CASE3(ST_MULF2)
  ST_CASE2(ST_SQ_C)
  ST_CASE2(ST_SQ_NC)
  ST_CASE2(ST_MUL_SMALL)
  ST_CASE2(ST_ADD)
  ST_CASE2(ST_SUB)
  ST_CASE2(ST_NEG)
  ST_CASE2(ST_SUB_LAZY)
  ST_CASE(ST_CARRY, 0)
  ST_CASE(ST_CANON, 0)
  ST_CASE(ST_FROM_WORDS, 0)
  ST_CASE(ST_INVERT_C, 0)
  ST_CASE(ST_INVERT_NC, 0)
  ST_CASE(ST_INVERT_VAR, 0)
  ST_CASE(ST_POW_C, 0)
  ST_CASE(ST_POW_NC, 0)
  ST_CASE(ST_SC_CANON, 0)
  ST_CASE(ST_SC_REDUCE, 0)
  ST_CASE(ST_FROMBYTES, 0)
  ST_CASE(ST_GE_DBL, 0)
  ST_CASE2(ST_GE_ADD)
#undef ST_CASE4
#undef ST_CASE3
#undef ST_CASE2
#undef ST_CASE
  if (op == ST_INVERT_VAR_WAVE && variant == 0) {
    hipLaunchKernelGGL(st_invert_wave_kernel, dim3(n), dim3(64), 0, 0, d_in, d_out, n);
    return true;
  }
  if (op == ST_FROMBYTES_ROW && variant == 0) {
    hipLaunchKernelGGL(st_frombytes_row_kernel, dim3((16 * n + 63) / 64), dim3(64), 0, 0, d_in, d_out, n);
    return true;
  }
  return false;
}

// Words read and written per case, and the number of variants, of operation op (0 for an unknown op).
extern "C" void fe25519_selftest_words(int op, int* in_words, int* out_words, int* variants) {
  const StWords w = st_words(op);
  *in_words = w.in;
  *out_words = w.out;
  *variants = w.variants;
}

// n cases of operation op in form variant: h_in holds n * in_words words, h_out takes n * out_words
// (fe25519_selftest_words).  Returns 0, a HIP error code, or -1 for an unknown (op, variant).
extern "C" int fe25519_selftest(int op, int variant, const uint32_t* h_in, uint32_t* h_out, int n) {
  const StWords w = st_words(op);
  if (w.in == 0 || variant < 0 || variant >= w.variants) return -1;
  if (n <= 0) return 0;
  const size_t in_bytes = (size_t)n * w.in * sizeof(uint32_t), out_bytes = (size_t)n * w.out * sizeof(uint32_t);
  uint32_t *d_in = nullptr, *d_out = nullptr;
  bool known = true;
  hipError_t e = hipMalloc(&d_in, in_bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes);
  if (e == hipSuccess) e = hipMemcpy(d_in, h_in, in_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, ST_SENTINEL_BYTE, out_bytes);
  if (e == hipSuccess) {
    known = st_dispatch(op, variant, d_in, d_out, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess && known) e = hipMemcpy(h_out, d_out, out_bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return known ? (int)e : -1;
}
