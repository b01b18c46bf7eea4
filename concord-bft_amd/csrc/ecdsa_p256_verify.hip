// ECDSA P-256 / SHA-256 batch verification kernels (gfx950).  The arithmetic is the lane code of
// ecdsa_p256_verify.h (one key, one message or one signature per lane); this file holds the three
// kernels and their launches.  The hash kernel is this file's own copy of the ecdsa_sha256 lane
// routine, so the secp256k1 object is not touched.
#include "ecdsa_p256_verify.h"

// one key per lane: validate, build the table of affine multiples
__global__ void __launch_bounds__(64) ecdsa_p256_keys_kernel(const uint8_t* pub, uint32_t nkeys, uint32_t* keys) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nkeys) return;
  ecdsa_p256_key_lane(keys + (size_t)k * ECDSA_KEY_WORDS, pub + (size_t)k * ECDSA_PUB_BYTES);
}

// one message per lane: digest words into the scratch.  The same text as ecdsa_hash_kernel of ecdsa_verify.hip
// (both are ecdsa_sha256 of ecdsa_verify.h around the same loads and stores): a change to one belongs in both.
__global__ void __launch_bounds__(64) ecdsa_p256_hash_kernel(const uint8_t* msg, const uint64_t* off,
                                                             const uint32_t* len, size_t n, uint32_t* digest) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t h[8];
  ecdsa_sha256(h, msg + off[i], len[i]);
#pragma unroll
  for (int j = 0; j < 8; j++) digest[i * 8 + j] = h[j];
}

// one signature per lane, one verdict word per wave
__global__ void __launch_bounds__(64) ecdsa_p256_verify_kernel(const EcdsaBatch b, const uint32_t* digest,
                                                               uint64_t* verdicts) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  bool ok = false;
  if (i < b.n) {
    const uint32_t k = b.key_idx[i];
    if (k < b.nkeys) {
      uint32_t h[8];
#pragma unroll
      for (int j = 0; j < 8; j++) h[j] = digest[i * 8 + j];
      ok = ecdsa_p256_verify_lane(b.keys + (size_t)k * ECDSA_KEY_WORDS, b.gtab, b.sig + i * ECDSA_SIG_BYTES, h);
    }
  }
  const uint64_t w = __ballot(ok);
  if (threadIdx.x == 0) verdicts[blockIdx.x] = w;
}

hipError_t cbft_ecdsa_p256_launch_keys(const uint8_t* d_pub, uint32_t nkeys, uint32_t* d_keys, hipStream_t stream) {
  if (nkeys == 0) return hipSuccess;
  ecdsa_p256_keys_kernel<<<dim3((nkeys + 63) / 64), dim3(64), 0, stream>>>(d_pub, nkeys, d_keys);
  return hipGetLastError();
}

hipError_t cbft_ecdsa_p256_launch_verify(const EcdsaBatch& b, uint32_t* d_scratch, uint64_t* d_verdicts,
                                         hipStream_t stream) {
  if (b.n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((b.n + 63) / 64);
  ecdsa_p256_hash_kernel<<<dim3(blocks), dim3(64), 0, stream>>>(b.msg, b.msg_off, b.msg_len, b.n, d_scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  ecdsa_p256_verify_kernel<<<dim3(blocks), dim3(64), 0, stream>>>(b, d_scratch, d_verdicts);
  return hipGetLastError();
}
