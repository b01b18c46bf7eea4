// Launch interface of the batched BLS BN-P254 multisig verification (bls_multisig_batch.hip, DESIGN.md
// §25): n independent checks e(g1_map(msg[msg_of[i]]), PK[set_of[i]]) == e(sigma_i, g2) where PK[j] is
// the sum of the key set's vk_id over the bits of signer bitmap j.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "bls_verify_batch.h"

// signer sets per call: bounds the scratch, which holds per set its 70 normalised lines (10,080 B), its
// affine sum (148 B) and one 220-byte partial sum per BLS_MULTISIG_CHUNK ids of the key set (at most
// 32 x 220 B), so at most 17.3 KB per set and 1.06 GiB per call.  More sets are CBFT_E2BIG.
#define BLS_MULTISIG_MAX_SETS (1u << 16)
// ids summed by one wave of the key-sum kernel
#define BLS_MULTISIG_CHUNK 64

struct BlsMultisigBatch {
  uint32_t n;               // items
  uint32_t m;               // messages
  uint32_t s;               // signer sets
  const uint8_t* signers;   // s x 256 bytes, bit id - 1 (LSB first) selects vk_id
  const uint32_t* set_of;   // n, or nullptr = item i uses set i
  const uint32_t* msg_of;   // n, or nullptr = item i signs message i
  const uint8_t* sig33;     // n x 33
  const uint8_t* msg;
  const uint64_t* off;  // m, or nullptr = fixed_len messages back to back
  const uint32_t* len;
  uint32_t fixed_len;
  uint32_t nkeys;           // vk_1 .. vk_nkeys: slots 1 .. nkeys of aff / key_ok (slot 0 is the group PK)
  const uint32_t* aff;      // (nkeys + 1) x BLS_G2A_WORDS
  const uint8_t* key_ok;    // nkeys + 1
  const uint32_t* gen_lines;
};

// bytes of scratch of the key sums of s sets over nkeys keys alone (cbft_bls_multisig_sum_launch)
size_t cbft_bls_multisig_sum_scratch_bytes(size_t s, uint32_t nkeys);
// bytes of scratch of a whole batch: the verification's own (bls_verify_batch.h) | per-set tables
size_t cbft_bls_multisig_batch_scratch_bytes(size_t n, size_t m, size_t s, uint32_t nkeys);
// Stage (a) alone: the s key sums.  d_out65 (s x 65) and d_ok (s) as cbft_bls_sum_keys gives them.
hipError_t cbft_bls_multisig_sum_launch(const BlsMultisigBatch& b, void* d_scratch, uint8_t* d_out65, uint8_t* d_ok,
                                        hipStream_t s);
// d_valid: n bytes, 1 = item verifies.  An item whose set or message index is out of range, whose set
// is empty, sums to infinity or selects a key that did not decode, or whose sigma does not decode gets
// 0 without running a pairing.
hipError_t cbft_bls_multisig_batch_launch(const BlsMultisigBatch& b, void* d_scratch, uint8_t* d_valid, hipStream_t s);
