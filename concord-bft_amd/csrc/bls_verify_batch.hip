// Batched BLS BN-P254 verification over many messages for gfx950: n independent
// checks e(g1_map(msg[msg_of[i]]), key[key_idx[i]]) == e(sigma_i, g2), each with an exact verdict.
//
//   blsv_decode_kernel    one DPP row per item (four per wave, bls_prep_kernel's decoding): sig33 -> the
//                         affine point (19 words) and the item's gate: sigma decoded, key slot in
//                         range and decoded, message index in range
//   bls_sign_hash_kernel  (bls_sign_batch.h) H = g1_map(msg) over the m MESSAGES into [word][m]
//   blsv_pair_kernel      one wave per item, both pairs on one Miller loop (p36_pairing_check<2>, <1>
//                         for an infinite sigma); H gathered from column msg_of[i], the key's lines
//                         from lines + key_idx[i] * LINES_PER_KEY.  A gated-out item costs its wave one
//                         byte load.
#include "bls_verify_batch.h"

#include "bls_common.h"
#include "bls_sign_batch.h"
#include "bn254_g2wave.h"
#include "bn254_pair36.h"

// scratch: H | sigma | gate flags
static __host__ __device__ inline size_t blsv_sig_at(size_t m) { return 2 * BN_LIMBS * m; }
static __host__ __device__ inline size_t blsv_gate_at(size_t n, size_t m) { return blsv_sig_at(m) + BLS_SIG_WORDS * n; }
size_t cbft_bls_verify_batch_scratch_bytes(size_t n, size_t m) { return blsv_gate_at(n, m) * sizeof(uint32_t) + n; }

__global__ void __launch_bounds__(64) blsv_decode_kernel(const uint8_t* sig33, const uint32_t* key_idx,
                                                         const uint32_t* msg_of, uint32_t n, uint32_t m,
                                                         uint32_t nkeys, const uint8_t* key_ok, uint32_t* sig,
                                                         uint8_t* gate) {
  const uint32_t j = blockIdx.x * 4 + ((threadIdx.x & 63) >> 4);
  const uint32_t jj = j < n ? j : n - 1;  // rows past the last item decode it again, store nothing
  g1a s;
  bool ok = g1_decompress_row(s, sig33 + 33 * (size_t)jj);
  const uint32_t ki = key_idx ? key_idx[jj] : 0u;
  const uint32_t mi = msg_of ? msg_of[jj] : jj;
  ok = ok && ki <= nkeys && mi < m;
  ok = ok && key_ok[ki] != 0;  // read only when the slot is in range
  if (j < n && (threadIdx.x & 15) == 0) {
    g1a_store(sig + BLS_SIG_WORDS * (size_t)j, s);
    gate[j] = ok ? 1 : 0;
  }
}

// Block i checks item i; the hardware hands out blocks as waves retire.  One wave owns lambda'
// (p36_lambda_x) for its two pairs: 2 x 70 x 54 words = 30,240 B of LDS.
__global__ void __launch_bounds__(64) blsv_pair_kernel(uint32_t n, uint32_t m, const uint32_t* key_idx,
                                                       const uint32_t* msg_of, const uint32_t* H,
                                                       const uint32_t* sig, const uint8_t* gate,
                                                       const uint32_t* lines, const uint32_t* gen_lines,
                                                       uint8_t* valid) {
  __shared__ uint32_t lxs[2 * BN_ATE_LINES * P36_LX_WORDS];
  const P36 g = p36_lane();
  const uint32_t i = blockIdx.x;
  if (i >= n) return;
  bool good = gate[i] != 0;  // wave-uniform
  if (good) {
    const uint32_t ki = key_idx ? key_idx[i] : 0u;
    const uint32_t mi = msg_of ? msg_of[i] : i;
    g1a P[2];
#pragma unroll
    for (int w = 0; w < BN_LIMBS; w++) {
      P[0].x.v[w] = H[(size_t)w * m + mi];
      P[0].y.v[w] = H[(size_t)(BN_LIMBS + w) * m + mi];
    }
    P[0].inf = false;
    g1a_load(P[1], sig + BLS_SIG_WORDS * (size_t)i);
    if (!P[1].inf) f_neg(P[1].y, P[1].y);
    const uint32_t* l[2] = {lines + (size_t)ki * LINES_PER_KEY, gen_lines};
    good = P[1].inf ? p36_pairing_check<1>(P, l, g, lxs) : p36_pairing_check<2>(P, l, g, lxs);
  }
  if (g.lane == 0) valid[i] = good ? 1 : 0;
}

hipError_t cbft_bls_verify_batch_launch(const BlsVerifyBatch& b, void* d_scratch, uint8_t* d_valid, hipStream_t s) {
  if (!b.n) return hipSuccess;
  uint32_t* w = static_cast<uint32_t*>(d_scratch);
  uint32_t* d_H = w;
  uint32_t* d_sig = w + blsv_sig_at(b.m);
  uint8_t* d_gate = reinterpret_cast<uint8_t*>(w + blsv_gate_at(b.n, b.m));
  hipLaunchKernelGGL(blsv_decode_kernel, dim3((b.n + 3) / 4), dim3(64), 0, s, b.sig33, b.key_idx, b.msg_of, b.n, b.m,
                     b.nkeys, b.key_ok, d_sig, d_gate);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (b.m) {
    hipLaunchKernelGGL(bls_sign_hash_kernel<true>, dim3((b.m + BLS_SIGN_HASH_CHUNK - 1) / BLS_SIGN_HASH_CHUNK), dim3(64),
                       0, s, b.msg, b.off, b.len, b.fixed_len, b.m, d_H, (uint32_t*)nullptr);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(blsv_pair_kernel, dim3(b.n), dim3(64), 0, s, b.n, b.m, b.key_idx, b.msg_of, d_H, d_sig, d_gate,
                     b.lines, b.gen_lines, d_valid);
  return hipGetLastError();
}
