// Batched, constant-time RSA-2048 PKCS#1 v1.5 / SHA-256 signing on gfx950.
//
// What it replaces: concord::util::crypto::RSASigner::sign (util/src/crypto_utils.cpp), the
// Crypto++ RSASS<PKCS1v15, SHA256>::Signer that SigManager holds for an RSA replica key, one
// signature at a time on the host.
//
// Two lanes per signature: the even lane computes m_p = EM^dP mod p, the odd lane m_q = EM^dQ mod q,
// each with whole 1,024-bit Montgomery products in registers (rsa_sign.h rs_mm: radix 2^28, 37
// limbs, no carries inside a product).  The lanes meet once, through DPP, for Garner's step.  The
// signatures then pass the public check s^e mod n == EM (the verify kernel of rsa_verify.hip, run
// by the C ABI layer) before they leave the device.
#include <hip/hip_runtime.h>

#define CBFT_RSA_SIGN_DEVICE_HELPERS
#include "rsa_sign.h"

namespace {

// EMSA-PKCS1-v1_5 representative for SHA-256 at 2048 bits, bytes 0..223 (the last 32 are the
// digest): 00 01 FF*202 00 || DigestInfo, in the layout of rsa_verify.hip's em_* helpers.
__device__ __forceinline__ uint32_t em_byte(int p) {
  const uint8_t di[19] = {0x30, 0x31, 0x30, 0x0d, 0x06, 0x09, 0x60, 0x86, 0x48, 0x01,
                          0x65, 0x03, 0x04, 0x02, 0x01, 0x05, 0x00, 0x04, 0x20};
  if (p == 0) return 0x00;
  if (p == 1) return 0x01;
  if (p < 204) return 0xff;
  if (p == 204) return 0x00;
  return di[p - 205];
}
// limb k (little-endian 32-bit) of the representative, 8 <= k < 64
__device__ __forceinline__ uint32_t em_limb(int k) {
  const int p = 252 - 4 * k;
  return (em_byte(p) << 24) | (em_byte(p + 1) << 16) | (em_byte(p + 2) << 8) | em_byte(p + 3);
}

// SHA-256 of msg[0..len) into eight big-endian state words (the message and its length are public)
__device__ __forceinline__ void sha256_words(uint32_t (&h)[8], const uint8_t* msg, uint32_t len) {
  h[0] = 0x6a09e667u, h[1] = 0xbb67ae85u, h[2] = 0x3c6ef372u, h[3] = 0xa54ff53au;
  h[4] = 0x510e527fu, h[5] = 0x9b05688cu, h[6] = 0x1f83d9abu, h[7] = 0x5be0cd19u;
  const uint32_t nblk = (len + 9 + 63) / 64;
  for (uint32_t bk = 0; bk < nblk; bk++) {
    uint32_t blk[16];
    const uint32_t base = 64 * bk;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      uint32_t w = 0;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t pos = base + 4 * j + q;
        const uint32_t byte = pos < len ? msg[pos] : (pos == len ? 0x80u : 0u);
        w = (w << 8) | byte;
      }
      blk[j] = w;
    }
    if (bk == nblk - 1) {
      blk[14] = len >> 29;
      blk[15] = len << 3;
    }
    sha256_block(h, blk);
  }
}

__global__ void __launch_bounds__(64) rsa_sign_keys_kernel(const uint8_t* priv, const uint32_t* exps, uint32_t nkeys,
                                                           uint32_t* recs, uint8_t* mod) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeys) return;
  rs_build_record(recs + (size_t)k * RSAS_WORDS, priv + (size_t)k * RSAS_PRIV_BYTES, exps[k], mod + (size_t)k * 256);
}

// Signatures base .. base + 32 gridDim.x of the batch.  Lanes past the batch's end and items with
// a signer index out of range work on item 0 / signer 0 and store nothing / are zeroed by the
// gate: every lane of every wave runs the same instructions.
__global__ void __launch_bounds__(64, 2) rsa_sign_kernel(const RsaSignBatch b, size_t base, uint32_t* scratch,
                                                      uint8_t* sig_out) {
  const uint32_t tid = threadIdx.x;
  const bool hi = tid & 1;
  const size_t sig = base + (size_t)blockIdx.x * RSAS_PSIG + (tid >> 1);
  const bool live = sig < b.n;
  const size_t si = live ? sig : 0;
  uint32_t kidx = b.signer_idx ? b.signer_idx[si] : 0u;
  if (kidx >= b.nkeys) kidx = 0;
  const uint32_t* rec = b.signers + (size_t)kidx * RSAS_WORDS;
  const uint8_t* msg = b.msg_off ? b.msg + b.msg_off[si] : b.msg + si * (size_t)b.fixed_len;
  const uint32_t len = b.msg_off ? b.msg_len[si] : b.fixed_len;

  uint32_t hw8[8], emw[64], em74[2 * RS_NL];
  sha256_words(hw8, msg, len);
#pragma unroll
  for (int k = 0; k < 64; k++) emw[k] = k < 8 ? hw8[7 - k] : em_limb(k);
#pragma unroll
  for (int i = 0; i < 2 * RS_NL; i++) em74[i] = rs_limb28<64>(emw, i);

  uint32_t s[64];
  rs_crt_core(s, rec, hi, em74, scratch + (size_t)blockIdx.x * (64 * RSAS_TBL * RSAS_NL) + tid);
  if (live && !hi) {
    uint32_t* out = reinterpret_cast<uint32_t*>(sig_out + sig * 256);
#pragma unroll
    for (int k = 0; k < 64; k++) out[63 - k] = __builtin_bswap32(s[k]);
  }
}

__global__ void __launch_bounds__(256) rsa_sign_prep_kernel(const RsaSignBatch b, uint32_t* idx, uint64_t* off,
                                                            uint32_t* len) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.n) return;
  const uint32_t k = b.signer_idx ? b.signer_idx[i] : 0u;
  idx[i] = k < b.nkeys ? k : 0u;
  off[i] = b.msg_off ? b.msg_off[i] : i * (uint64_t)b.fixed_len;
  len[i] = b.msg_off ? b.msg_len[i] : b.fixed_len;
}

__global__ void __launch_bounds__(256) rsa_sign_gate_kernel(const RsaSignBatch b, const uint64_t* verdicts,
                                                            int use_status, uint8_t* sig, uint32_t* failed) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.n) return;
  const uint32_t k = b.signer_idx ? b.signer_idx[i] : 0u;
  const bool in_range = k < b.nkeys;
  bool good = in_range && ((verdicts[i >> 6] >> (i & 63)) & 1ull);
  if (good && use_status) good = b.signers[(size_t)k * RSAS_WORDS + RSAS_STATUS] == 1u;
  if (good) return;
  uint32_t* out = reinterpret_cast<uint32_t*>(sig + i * 256);
  for (int w = 0; w < 64; w++) out[w] = 0u;
  if (in_range && failed) atomicAdd(failed, 1u);
}

__global__ void __launch_bounds__(64) rsa_sign_status_kernel(uint32_t* recs, uint32_t nkeys, const uint64_t* verdicts) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeys) return;
  uint32_t* rec = recs + (size_t)k * RSAS_WORDS;
  rec[RSAS_STATUS] = (rec[RSAS_STRUCT] == 1u && ((verdicts[k >> 6] >> (k & 63)) & 1ull)) ? 1u : 0u;
}

size_t blocks_of(size_t n) { return (n + RSAS_PSIG - 1) / RSAS_PSIG; }

}  // namespace

size_t cbft_rsa_sign_scratch_words(size_t n) {
  const size_t m = n < RSAS_MAX_LAUNCH ? n : (size_t)RSAS_MAX_LAUNCH;
  return blocks_of(m) * 64 * RSAS_TBL * RSAS_NL;
}

hipError_t cbft_rsa_sign_launch_keys(const uint8_t* d_priv, const uint32_t* d_exp, uint32_t nkeys,
                                     uint32_t* d_signers, uint8_t* d_mod, hipStream_t stream) {
  if (!nkeys) return hipSuccess;
  hipLaunchKernelGGL(rsa_sign_keys_kernel, dim3((nkeys + 63) / 64), dim3(64), 0, stream, d_priv, d_exp, nkeys,
                     d_signers, d_mod);
  return hipGetLastError();
}

hipError_t cbft_rsa_sign_launch(const RsaSignBatch& b, uint32_t* d_scratch, uint8_t* d_sig, hipStream_t stream) {
  // launches of one batch follow each other on the stream and share the scratch
  for (size_t base = 0; base < b.n; base += RSAS_MAX_LAUNCH) {
    const size_t m = b.n - base < RSAS_MAX_LAUNCH ? b.n - base : (size_t)RSAS_MAX_LAUNCH;
    hipLaunchKernelGGL(rsa_sign_kernel, dim3((unsigned)blocks_of(m)), dim3(64), 0, stream, b, base, d_scratch, d_sig);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t cbft_rsa_sign_launch_prep(const RsaSignBatch& b, uint32_t* d_idx, uint64_t* d_off, uint32_t* d_len,
                                     hipStream_t stream) {
  if (!b.n) return hipSuccess;
  hipLaunchKernelGGL(rsa_sign_prep_kernel, dim3((unsigned)((b.n + 255) / 256)), dim3(256), 0, stream, b, d_idx, d_off,
                     d_len);
  return hipGetLastError();
}

hipError_t cbft_rsa_sign_launch_gate(const RsaSignBatch& b, const uint64_t* d_verdicts, int use_status,
                                     uint8_t* d_sig, uint32_t* d_failed, hipStream_t stream) {
  if (!b.n) return hipSuccess;
  hipLaunchKernelGGL(rsa_sign_gate_kernel, dim3((unsigned)((b.n + 255) / 256)), dim3(256), 0, stream, b, d_verdicts,
                     use_status, d_sig, d_failed);
  return hipGetLastError();
}

hipError_t cbft_rsa_sign_launch_status(uint32_t* d_signers, uint32_t nkeys, const uint64_t* d_verdicts,
                                       hipStream_t stream) {
  if (!nkeys) return hipSuccess;
  hipLaunchKernelGGL(rsa_sign_status_kernel, dim3((nkeys + 63) / 64), dim3(64), 0, stream, d_signers, nkeys,
                     d_verdicts);
  return hipGetLastError();
}
