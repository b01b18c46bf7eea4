// Host-side pieces that every front end of libcbft_hipcrypto (cbft_*.cpp) shares and that need no
// GPU: wiping secrets, the blob range a batch's messages span, the packed input image's layout and
// the verdict words -> bitmap copy.  No HIP here: tests/cpp/host_util_test.cpp builds this header
// alone with g++ under ASan + UBSan.  The helpers that issue HIP calls are in cbft_internal.h.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

// memset the optimiser may not drop
inline void cbft_wipe(void* p, size_t n) {
  volatile uint8_t* v = static_cast<volatile uint8_t*>(p);
  for (size_t i = 0; i < n; i++) v[i] = 0;
}

// The blob range [lo, lo + blob) that a batch's m messages span: only that range moves to the
// device, with the offsets rebased to it (a shard of a multi-GPU batch carries its own part of the
// caller's blob).  Failures, all CBFT_EINVAL to the caller: LEN a message longer than max_len
// (0 = no cap), WRAP msg_off[i] + msg_len[i] passes 2^64, NO_BLOB a span that is not empty with no
// blob to read it from.  The first one met, in message order, is returned and nothing is written;
// otherwise `rebased` holds the m values msg_off[i] - lo.
enum CbftSpanError { CBFT_SPAN_OK = 0, CBFT_SPAN_LEN, CBFT_SPAN_WRAP, CBFT_SPAN_NO_BLOB };
struct CbftSpan {
  CbftSpanError err = CBFT_SPAN_OK;
  uint64_t lo = 0, blob = 0;
};
inline CbftSpan cbft_msg_span(const uint64_t* msg_off, const uint32_t* msg_len, size_t m, uint32_t max_len,
                              bool have_blob, uint64_t* rebased) {
  uint64_t lo = UINT64_MAX, hi = 0;
  for (size_t i = 0; i < m; i++) {
    if (max_len && msg_len[i] > max_len) return {CBFT_SPAN_LEN};
    if (msg_off[i] > UINT64_MAX - msg_len[i]) return {CBFT_SPAN_WRAP};
    lo = std::min<uint64_t>(lo, msg_off[i]);
    hi = std::max<uint64_t>(hi, msg_off[i] + msg_len[i]);
  }
  if (hi > lo && !have_blob) return {CBFT_SPAN_NO_BLOB};
  for (size_t i = 0; i < m; i++) rebased[i] = msg_off[i] - lo;
  return {CBFT_SPAN_OK, lo, hi > lo ? hi - lo : 0};
}

// One packed device image of a host-array batch:
//   offsets (m x 8, rebased) | lengths (m x 4) | up to CBFT_PACKED_MID per-item arrays | blob | 16 bytes
// The middle arrays are the signer indices of a signing batch, or the key slots, message indices and
// signatures of a BLS verification batch.  The 16 bytes after the blob let the hash kernels read
// whole words past a message's end.
#define CBFT_PACKED_MID 3
struct CbftPackedArray {  // a middle array as the caller holds it; host == nullptr: the caller gave none
  const void* host;
  size_t bytes;
};
struct CbftPackedLayout {
  size_t off = 0, len = 0, mid[CBFT_PACKED_MID] = {}, blob = 0, bytes = 0;
};
inline CbftPackedLayout cbft_packed_layout(size_t m, const CbftPackedArray* mid, size_t n_mid, uint64_t blob) {
  CbftPackedLayout L;
  L.len = m * 8;
  L.blob = L.len + m * 4;
  for (size_t k = 0; k < n_mid && k < CBFT_PACKED_MID; k++) {
    L.mid[k] = L.blob;
    L.blob += mid[k].bytes;
  }
  L.bytes = L.blob + blob + 16;
  return L;
}

// ceil(n / 64) verdict words (bit i of the batch = bit i % 64 of word i / 64; a little-endian host,
// so words == bytes) -> the caller's bitmap of ceil(n / 8) bytes, the bits from n on cleared
inline void cbft_verdicts_to_bitmap(uint8_t* bitmap, const uint64_t* words, size_t n) {
  const size_t nbytes = (n + 7) / 8;
  std::copy_n(reinterpret_cast<const uint8_t*>(words), nbytes, bitmap);
  if (n % 8) bitmap[nbytes - 1] &= (uint8_t)((1u << (n % 8)) - 1);
}
