// Test-only device harness (not part of the product library): the P-256 lane routines of
// csrc/fe_p256.h, sc_p256.h and ge_p256.h for chosen inputs, one function per launch and one lane per
// input, so tests/test_ecdsa_p256_lane_gpu.py can compare every output word on gfx950 with Python
// integers: a device-only miscompile, or a carry that the verdict bit of a whole verification hides.
//
// Operands are 8 little-endian words each (five arrays a..e); every lane writes EPS_OUT words:
//   [0..8) first result, [8..16) second result, [16] flag, [17..24) zero.
#include <hip/hip_runtime.h>

#include "ecdsa_p256_verify.h"

#define EPS_OUT 24
#define EPS_OPS 10

struct EpsIn {
  const uint32_t *a, *b, *c, *d, *e;
};

__device__ __forceinline__ void eps_load(uint32_t* r, const uint32_t* p, int i) {
#pragma unroll
  for (int j = 0; j < 8; j++) r[j] = p[8 * i + j];
}
__device__ __forceinline__ void eps_put(uint32_t* out, int i, const uint32_t* a, const uint32_t* b, uint32_t flag) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    out[EPS_OUT * i + j] = a[j];
    out[EPS_OUT * i + 8 + j] = b[j];
    out[EPS_OUT * i + 16 + j] = j == 0 ? flag : 0u;
  }
}
// (x, y) scaled to Jacobian coordinates with z (z != 0)
__device__ __forceinline__ void eps_jac(P2Jac& p, const P2Fe& x, const P2Fe& y, const P2Fe& z) {
  P2Fe z2;
  p2_fe_sqr(z2, z);
  p2_fe_mul(p.x, x, z2);
  p2_fe_mul(z2, z2, z);
  p2_fe_mul(p.y, y, z2);
  p.z = z;
}

// OP: 0 fe_mul(a, b)  1 fe_sqr(a)  2 fe_add(a, b)  3 fe_sub(a, b)      (a, b < p)
//     4 flag = fe_eq(a, b) | fe_is_zero(a) << 1 | fe_from_be's range test of a's words << 2; first = reduce512(a b)
//       for ANY 256-bit a, b
//     5 sc_mul(a, b) for ANY 256-bit a, b; second = a mod n; flag = a < n
//     6 fe_inv_var(a)  7 sc_inv_var(a)
//     8 ge_dbl of (a, b) scaled by c: affine result, flag 1 = infinity
//     9 ge_madd of (a, b) scaled by c, plus the affine (d, e); c = 0: the first operand is infinity
template <int OP>
__global__ void __launch_bounds__(64) eps_kernel(const EpsIn in, uint32_t* out, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  P2Fe a, b, r;
  eps_load(a.v, in.a, i);
  eps_load(b.v, in.b, i);
  if (OP <= 3) {
    if (OP == 0) p2_fe_mul(r, a, b);
    if (OP == 1) p2_fe_sqr(r, a);
    if (OP == 2) p2_fe_add(r, a, b);
    if (OP == 3) p2_fe_sub(r, a, b);
    eps_put(out, i, r.v, zero, 0);
  } else if (OP == 4) {
    const uint32_t P[8] = P2_P_LIMBS;
    uint32_t w[16], u[8];
    k1_mul512(w, a.v, b.v);
    p2_fe_reduce512(r, w);
    const uint32_t below = k1_sub256(u, a.v, P);
    eps_put(out, i, r.v, zero, (p2_fe_eq(a, b) ? 1u : 0u) | (p2_fe_is_zero(a) ? 2u : 0u) | (below ? 4u : 0u));
  } else if (OP == 5) {
    P2Sc x, y, m, red;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      x.v[j] = a.v[j];
      y.v[j] = b.v[j];
    }
    p2_sc_mul(m, x, y);
    p2_sc_reduce256(red, x.v);
    eps_put(out, i, m.v, red.v, p2_sc_in_range(x.v) ? 1u : 0u);
  } else if (OP == 6) {
    p2_fe_inv_var(r, a);
    eps_put(out, i, r.v, zero, 0);
  } else if (OP == 7) {
    P2Sc x, w;
#pragma unroll
    for (int j = 0; j < 8; j++) x.v[j] = a.v[j];
    p2_sc_inv_var(w, x);
    eps_put(out, i, w.v, zero, 0);
  } else {
    P2Fe z;
    eps_load(z.v, in.c, i);
    P2Jac p, q;
    if (p2_fe_is_zero(z)) {
      p2_ge_set_inf(p);
    } else {
      eps_jac(p, a, b, z);
    }
    if (OP == 8) {
      p2_ge_dbl(q, p);
    } else {
      P2Aff t;
      eps_load(t.x.v, in.d, i);
      eps_load(t.y.v, in.e, i);
      p2_ge_madd(q, p, t);
    }
    if (p2_ge_is_inf(q)) {
      eps_put(out, i, zero, zero, 1);
    } else {
      P2Aff o;
      p2_ge_to_aff(o, q);
      eps_put(out, i, o.x.v, o.y.v, 0);
    }
  }
}

template <int OP>
static void eps_launch(const EpsIn& in, uint32_t* d_out, int n) {
  hipLaunchKernelGGL(eps_kernel<OP>, dim3((n + 63) / 64), dim3(64), 0, 0, in, d_out, n);
}

// h_in: five arrays of n x 8 words, one after the other; h_out: n x EPS_OUT words (sent to the device first,
// so a lane that writes nothing leaves the caller's sentinel).  Returns the hipError_t, or -1 for a bad call.
extern "C" int ecdsa_p256_selftest(int op, const uint32_t* h_in, uint32_t* h_out, int n) {
  if (n <= 0 || n > (1 << 16) || op < 0 || op >= EPS_OPS) return -1;
  const size_t bytes = (size_t)n * 8 * 4, obytes = (size_t)n * EPS_OUT * 4;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, 5 * bytes);
  if (e == hipSuccess) e = hipMalloc(&d_out, obytes);
  if (e == hipSuccess) e = hipMemcpy(d_in, h_in, 5 * bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_out, h_out, obytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const size_t w = (size_t)n * 8;
    const EpsIn in{d_in, d_in + w, d_in + 2 * w, d_in + 3 * w, d_in + 4 * w};
    switch (op) {
      case 0: eps_launch<0>(in, d_out, n); break;
      case 1: eps_launch<1>(in, d_out, n); break;
      case 2: eps_launch<2>(in, d_out, n); break;
      case 3: eps_launch<3>(in, d_out, n); break;
      case 4: eps_launch<4>(in, d_out, n); break;
      case 5: eps_launch<5>(in, d_out, n); break;
      case 6: eps_launch<6>(in, d_out, n); break;
      case 7: eps_launch<7>(in, d_out, n); break;
      case 8: eps_launch<8>(in, d_out, n); break;
      default: eps_launch<9>(in, d_out, n); break;
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h_out, d_out, obytes, hipMemcpyDeviceToHost);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return (int)e;
}
