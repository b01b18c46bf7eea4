// Host build of the fixed-length SHA-512 front end (concord-bft_amd/csrc/sha512.h: sha512_ram_fixed,
// that is sha512_fixed_window + sha512_words_le + sha512_compress), exposed to the Python tests
// through ctypes: the SAME source that runs on gfx950, with plain C++ stand-ins for the three GPU
// builtins, checked on the CPU against hashlib.sha512.  Test infrastructure.
#include <cstdint>
#include <cstring>
#include <vector>

#include "sha512.h"

// digest (64 bytes, as SHA-512 prints it) of R || A || M; R, A: 32 bytes each; M: len bytes, len a
// multiple of 4.  The message is copied into a buffer of exactly len bytes, so a read past its end
// is a heap overflow that a sanitizer build reports.
extern "C" int sha512_shim_ram_fixed(const uint8_t* R, const uint8_t* A, const uint8_t* M, uint32_t len, uint8_t* out) {
  if (len % 4) return -1;
  uint32_t Rw[8], Aw[8], dig[16];
  std::memcpy(Rw, R, 32);
  std::memcpy(Aw, A, 32);
  uint32_t* m = new uint32_t[len / 4];  // non-null also for len == 0
  if (len) std::memcpy(m, M, len);
  sha512_ram_fixed(dig, Rw, Aw, m, len);
  delete[] m;
  std::memcpy(out, dig, 64);  // dig: the digest's bytes as little-endian words
  return 0;
}

// the general (byte-wise) routine of the same header, for comparison
extern "C" void sha512_shim_ram(const uint8_t* R, const uint8_t* A, const uint8_t* M, uint32_t len, uint8_t* out) {
  uint32_t Rw[8], Aw[8], dig[16];
  std::memcpy(Rw, R, 32);
  std::memcpy(Aw, A, 32);
  std::vector<uint8_t> m(M, M + len);
  sha512_ram(dig, Rw, Aw, m.data(), len);
  std::memcpy(out, dig, 64);
}

#ifdef SHA512_SHIM_MAIN
// Stand-alone run for sanitizer builds (-fsanitize=address,undefined): every length 0, 4, ..., 400
// through both routines; they must agree.  Exit status 0 = agree (and the sanitizer found nothing).
#include <cstdio>
int main() {
  uint8_t R[32], A[32], M[400], a[64], b[64];
  uint32_t x = 0x9e3779b9u;
  auto next = [&] { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return (uint8_t)(x >> 11); };
  for (uint32_t len = 0; len <= 400; len += 4) {
    for (auto& v : R) v = next();
    for (auto& v : A) v = next();
    for (uint32_t i = 0; i < len; i++) M[i] = next();
    if (sha512_shim_ram_fixed(R, A, M, len, a) != 0) return 2;
    sha512_shim_ram(R, A, M, len, b);
    if (std::memcmp(a, b, 64) != 0) {
      std::printf("mismatch at len %u\n", len);
      return 1;
    }
  }
  std::printf("sha512_ram_fixed == sha512_ram for len 0, 4, ..., 400\n");
  return 0;
}
#endif
