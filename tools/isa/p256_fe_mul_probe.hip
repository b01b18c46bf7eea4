// ISA probe of the P-256 field product: the same 8 x 8 limb product reduced by the
// word-wise Solinas sum that fe_p256.h keeps (k_solinas) and by a word-by-word Montgomery reduction
// (k_mont: p = -1 mod 2^32, so the quotient word is the low word and m p is four shifted adds).  Not part
// of any build; count v_mad_u64_u32 against all vector instructions of each kernel in
//   hipcc -S --cuda-device-only --offload-arch=gfx950 -O3 -std=c++17 -Iconcord-bft_amd/csrc tools/isa/p256_fe_mul_probe.hip   (make p256_isa)
#include "p256_mont_sketch.h"

__global__ void k_solinas(const uint32_t* a, const uint32_t* b, uint32_t* o) {
  P2Fe x, y, r;
  for (int i = 0; i < 8; i++) { x.v[i] = a[threadIdx.x * 8 + i]; y.v[i] = b[threadIdx.x * 8 + i]; }
  p2_fe_mul(r, x, y);
  for (int i = 0; i < 8; i++) o[threadIdx.x * 8 + i] = r.v[i];
}
__global__ void k_mont(const uint32_t* a, const uint32_t* b, uint32_t* o) {
  P2Fe x, y, r;
  for (int i = 0; i < 8; i++) { x.v[i] = a[threadIdx.x * 8 + i]; y.v[i] = b[threadIdx.x * 8 + i]; }
  uint32_t w[16];
  k1_mul512(w, x.v, y.v);
  mont_reduce512(r, w);
  for (int i = 0; i < 8; i++) o[threadIdx.x * 8 + i] = r.v[i];
}
