// Launch interface of the batched BLS BN-P254 verification (bls_verify_batch.hip):
// n independent pairing checks, each with its own message and its own key slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// items per call: keeps every index (19 n, 33 n, 18 m words) far inside 32-bit grids
#define BLS_VERIFY_BATCH_MAX (1u << 26)

struct BlsVerifyBatch {
  uint32_t n;               // items
  uint32_t m;               // messages
  const uint32_t* key_idx;  // n, or nullptr = slot 0 (the group PK)
  const uint32_t* msg_of;   // n, or nullptr = item i signs message i
  const uint8_t* sig33;     // n x 33
  const uint8_t* msg;
  const uint64_t* off;  // m, or nullptr = fixed_len messages back to back
  const uint32_t* len;
  uint32_t fixed_len;
  uint32_t nkeys;           // slots 0 .. nkeys of the key set
  const uint32_t* lines;    // (nkeys + 1) x lines-per-key words
  const uint8_t* key_ok;    // nkeys + 1
  const uint32_t* gen_lines;
};

// bytes of scratch for a batch of n items over m messages: H [18][m] | sigma 19 n | gate flags n
size_t cbft_bls_verify_batch_scratch_bytes(size_t n, size_t m);
// d_valid: n bytes, 1 = item verifies.  An item whose key slot or message index is out of range, whose
// key did not decode or whose sigma does not decode gets 0 without running a pairing.
hipError_t cbft_bls_verify_batch_launch(const BlsVerifyBatch& b, void* d_scratch, uint8_t* d_valid, hipStream_t s);
