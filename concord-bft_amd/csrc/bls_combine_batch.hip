// Batched BLS BN-P254 share combination over many certificates for gfx950: m
// certificates of a few shares each, one share per lane, so that m k shares fill the chip whatever k is.
//
//   blsc_decode_kernel    one DPP row per share (four per wave, blsv_decode_kernel's decoding): share37 ->
//                         id, the id in Montgomery form mod r, the affine point (19 words) and the
//                         share's state (unused / good / bad)
//   blsc_lagrange_kernel  one lane per share: walks the good ids of its own certificate
//                         (blsc_lagrange_lane): lambda_i, and a repeated id closes the certificate.
//                         Multisig runs the id walk alone.
//   blsc_mul_kernel       one lane per share: lambda_i sigma_i (blsc_mul_lane), the window table in LDS.
//                         Multisig skips it.
//   blsc_wave_sum_kernel  one lane per share: a segmented butterfly over the wave (log2 64 steps of complete
//                         additions, a step running only while some lane still has a partner in its own
//                         certificate) leaves in the first lane of every certificate segment that
//                         segment's sum and the OR of its flags
//   blsc_finish_kernel    one lane per certificate: the sum of its segments (one for a certificate inside
//                         a wave, at most k / 64 + 2), one inversion, compression, status
#include "bls_combine_batch.h"

#include "bls_common.h"

// scratch words: sigma 19 n | ids n | ids mod r 9 n | lambda 8 n | products 27 n | flags n ; then n state bytes
static __host__ __device__ inline size_t blsc_ids_at(size_t n) { return BLS_SIG_WORDS * n; }
static __host__ __device__ inline size_t blsc_idm_at(size_t n) { return blsc_ids_at(n) + n; }
static __host__ __device__ inline size_t blsc_lam_at(size_t n) { return blsc_idm_at(n) + BN_LIMBS * n; }
static __host__ __device__ inline size_t blsc_prod_at(size_t n) { return blsc_lam_at(n) + 8 * n; }
static __host__ __device__ inline size_t blsc_flag_at(size_t n) { return blsc_prod_at(n) + BLS_JAC_WORDS * n; }
static __host__ __device__ inline size_t blsc_state_at(size_t n) { return blsc_flag_at(n) + n; }
size_t cbft_bls_combine_batch_scratch_bytes(size_t n) { return blsc_state_at(n) * sizeof(uint32_t) + n; }

// the certificate of share i: i / k, or the last c with off[c] <= i (empty certificates own nothing)
__device__ __forceinline__ uint32_t blsc_cert_of(uint32_t i, const uint32_t* off, uint32_t k, uint32_t m) {
  if (!off) return i / k;
  uint32_t lo = 0, hi = m;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
__device__ __forceinline__ void blsc_cert_range(uint32_t& lo, uint32_t& hi, uint32_t c, const uint32_t* off,
                                                uint32_t k) {
  lo = off ? off[c] : c * k;
  hi = off ? off[c + 1] : lo + k;
}

__global__ void __launch_bounds__(64) blsc_decode_kernel(const uint8_t* shares, const uint8_t* use, uint32_t n,
                                                         uint32_t* sig, uint32_t* ids, uint32_t* idm, uint8_t* state) {
  const uint32_t j = blockIdx.x * 4 + ((threadIdx.x & 63) >> 4);
  const uint32_t jj = j < n ? j : n - 1;  // rows past the last share decode it again, store nothing
  const bool used = use ? use[jj] != 0 : true;
  uint32_t id = 0;
  g1a s;
  s.inf = true;
  bool ok = false;
  if (__any(used)) ok = bls_parse_share_row(id, s, shares + 37 * (size_t)jj);  // the whole wave, or none of it
  if (j < n && (threadIdx.x & 15) == 0) {
    const uint8_t st = !used ? BLSC_UNUSED : (ok && id >= 1 && id <= BLS_COMBINE_MAX_K ? BLSC_GOOD : BLSC_BAD);
    state[j] = st;
    if (st == BLSC_GOOD) {
      g1a_store(sig + BLS_SIG_WORDS * (size_t)j, s);
      ids[j] = id;
      const uint32_t w[8] = {id, 0, 0, 0, 0, 0, 0, 0};
      fr t;
      f_from_words(t, w);
      for (int q = 0; q < BN_LIMBS; q++) idm[BN_LIMBS * (size_t)j + q] = t.v[q];
    }
  }
}

__global__ void __launch_bounds__(64) blsc_lagrange_kernel(uint32_t n, uint32_t m, const uint32_t* off, uint32_t k,
                                                           int multisig, const uint32_t* ids, const uint32_t* idm,
                                                           const uint8_t* state, const uint32_t* inv, uint32_t* lam,
                                                           uint32_t* flag) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint8_t st = state[i];
  uint32_t f = st == BLSC_UNUSED ? 0u : BLSC_F_USED;
  if (st == BLSC_BAD) f |= BLSC_F_BAD;
  if (st == BLSC_GOOD) {
    uint32_t lo, hi, l8[8];
    blsc_cert_range(lo, hi, blsc_cert_of(i, off, k, m), off, k);
    if (blsc_lagrange_lane(l8, ids, idm, state, lo, hi, i, inv, multisig != 0))
      f |= BLSC_F_BAD;
    else if (!multisig)
      for (int q = 0; q < 8; q++) lam[8 * (size_t)i + q] = l8[q];
  }
  flag[i] = f;
}

// the four Jacobian table entries of a share in LDS, [entry][word][lane]: 27 KB per wave.  Held to the
// 256 registers of two waves per SIMD (the addition it calls takes 248)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) blsc_mul_kernel(uint32_t n, const uint32_t* sig, const uint32_t* lam,
                                                      const uint8_t* state, const uint32_t* flag, uint32_t* prod) {
  __shared__ uint32_t lds[BLS_SIGN_TBL_WORDS(BLSC_W) * 64];
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n || state[i] != BLSC_GOOD || (flag[i] & BLSC_F_BAD)) return;  // a repeated id left no lambda
  g1a P;
  g1a_load(P, sig + BLS_SIG_WORDS * (size_t)i);
  uint32_t l8[8];
  for (int q = 0; q < 8; q++) l8[q] = lam[8 * (size_t)i + q];
  BlsTblStrided t{lds + threadIdx.x, (size_t)64};
  g1j R;
  blsc_mul_lane(R, P, l8, t);
#pragma unroll
  for (int w = 0; w < BN_LIMBS; w++) {
    prod[(size_t)w * n + i] = R.X.v[w];
    prod[(size_t)(9 + w) * n + i] = R.Y.v[w];
    prod[(size_t)(18 + w) * n + i] = R.Z.v[w];
  }
}

__global__ void __launch_bounds__(64) blsc_wave_sum_kernel(uint32_t n, uint32_t m, const uint32_t* off, uint32_t k,
                                                           int multisig, const uint32_t* sig, const uint8_t* state,
                                                           uint32_t* prod, uint32_t* flag) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 64u + lane;
  const bool live = i < n;
  const uint32_t cert = live ? blsc_cert_of(i, off, k, m) : 0xffffffffu;
  uint32_t f = live ? flag[i] : 0u;
  g1j acc;
  g1_set_inf(acc);
  if (live && state[i] == BLSC_GOOD && !(f & BLSC_F_BAD)) {
    if (multisig) {
      g1a a;
      g1a_load(a, sig + BLS_SIG_WORDS * (size_t)i);
      g1_from_affine(acc, a);
    } else {
#pragma unroll
      for (int w = 0; w < BN_LIMBS; w++) {
        acc.X.v[w] = prod[(size_t)w * n + i];
        acc.Y.v[w] = prod[(size_t)(9 + w) * n + i];
        acc.Z.v[w] = prod[(size_t)(18 + w) * n + i];
      }
    }
  }
#pragma unroll 1
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t oc = (uint32_t)__shfl_down((int)cert, d);
    const bool has = live && lane + d < 64 && oc == cert;
    // segments are contiguous: nobody has a partner at distance 2 d when nobody has one at d
    if (!__any(has)) break;
    g1j o;
#pragma unroll
    for (int w = 0; w < BN_LIMBS; w++) {
      o.X.v[w] = (uint32_t)__shfl_down((int)acc.X.v[w], d);
      o.Y.v[w] = (uint32_t)__shfl_down((int)acc.Y.v[w], d);
      o.Z.v[w] = (uint32_t)__shfl_down((int)acc.Z.v[w], d);
    }
    const uint32_t of = (uint32_t)__shfl_down((int)f, d);
    if (has) {
      g1j t;
      blsc_add(t, acc, o);
      acc = t;
      f |= of;
    }
  }
  const uint32_t pc = (uint32_t)__shfl_up((int)cert, 1);
  if (live && (lane == 0 || pc != cert)) {
#pragma unroll
    for (int w = 0; w < BN_LIMBS; w++) {
      prod[(size_t)w * n + i] = acc.X.v[w];
      prod[(size_t)(9 + w) * n + i] = acc.Y.v[w];
      prod[(size_t)(18 + w) * n + i] = acc.Z.v[w];
    }
    flag[i] = f;
  }
}

__global__ void __launch_bounds__(64) blsc_finish_kernel(uint32_t n, uint32_t m, const uint32_t* off, uint32_t k,
                                                         const uint32_t* prod, const uint32_t* flag, uint8_t* out33,
                                                         uint8_t* status) {
  const uint32_t c = blockIdx.x * 64u + threadIdx.x;
  if (c >= m) return;
  uint32_t lo, hi;
  blsc_cert_range(lo, hi, c, off, k);
  // segment q of the certificate starts at lo (q = 0) or at the q-th multiple of 64 after lo
  const uint32_t np = lo == hi ? 0u : 1u + ((hi - 1) / 64u - lo / 64u);
  auto at = [lo](uint32_t q) { return q ? (lo / 64u + q) * 64u : lo; };
  uint32_t f = 0;
  for (uint32_t q = 0; q < np; q++) f |= flag[at(q)];
  blsc_finish(out33 + 33 * (size_t)c, status + c, f, np, [&](g1j& p, uint32_t q) {
    const uint32_t i = at(q);
#pragma unroll
    for (int w = 0; w < BN_LIMBS; w++) {
      p.X.v[w] = prod[(size_t)w * n + i];
      p.Y.v[w] = prod[(size_t)(9 + w) * n + i];
      p.Z.v[w] = prod[(size_t)(18 + w) * n + i];
    }
  });
}

hipError_t cbft_bls_combine_batch_launch(const BlsCombineBatch& b, void* d_scratch, hipStream_t s, hipEvent_t* ev) {
  if (!b.m) return hipSuccess;
  const size_t n = b.n;
  uint32_t* w = static_cast<uint32_t*>(d_scratch);
  uint32_t* d_sig = w;
  uint32_t* d_ids = w + blsc_ids_at(n);
  uint32_t* d_idm = w + blsc_idm_at(n);
  uint32_t* d_lam = w + blsc_lam_at(n);
  uint32_t* d_prod = w + blsc_prod_at(n);
  uint32_t* d_flag = w + blsc_flag_at(n);
  uint8_t* d_state = reinterpret_cast<uint8_t*>(w + blsc_state_at(n));
  hipError_t e = hipSuccess;
  auto mark = [&](int i) { return ev ? hipEventRecord(ev[i], s) : hipSuccess; };
  if ((e = mark(0)) != hipSuccess) return e;
  const dim3 lanes((b.n + 63) / 64);
  if (b.n) {
    hipLaunchKernelGGL(blsc_decode_kernel, dim3((b.n + 3) / 4), dim3(64), 0, s, b.shares, b.use, b.n, d_sig, d_ids, d_idm,
                       d_state);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = mark(1)) != hipSuccess) return e;
  if (b.n) {
    hipLaunchKernelGGL(blsc_lagrange_kernel, lanes, dim3(64), 0, s, b.n, b.m, b.off, b.k, b.multisig, d_ids, d_idm, d_state,
                       b.inv, d_lam, d_flag);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = mark(2)) != hipSuccess) return e;
  if (b.n && !b.multisig) {
    hipLaunchKernelGGL(blsc_mul_kernel, lanes, dim3(64), 0, s, b.n, d_sig, d_lam, d_state, d_flag, d_prod);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = mark(3)) != hipSuccess) return e;
  if (b.n) {
    hipLaunchKernelGGL(blsc_wave_sum_kernel, lanes, dim3(64), 0, s, b.n, b.m, b.off, b.k, b.multisig, d_sig, d_state,
                       d_prod, d_flag);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(blsc_finish_kernel, dim3((b.m + 63) / 64), dim3(64), 0, s, b.n, b.m, b.off, b.k, d_prod, d_flag,
                     b.out33, b.status);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return mark(4);
}
