// Batched BLS BN-P254 multisig verification over many signer sets for gfx950: n
// independent checks e(g1_map(msg[msg_of[i]]), PK[set_of[i]]) == e(sigma_i, g2), PK[j] = sum of vk_id over
// the bits of bitmap j, each with an exact verdict.  Everything is public key material: nothing here is
// constant time.
//
//   blsm_sum_part_kernel  one wave per (set, chunk of BLS_MULTISIG_CHUNK ids): the selected keys of the
//                         chunk by mixed additions on row-parallel Fp (g2r_accum_aff: exact for a doubling,
//                         a point and its negative, an infinite running sum) -> one partial per chunk
//   blsm_sum_fin_kernel   one wave per set: the set's partials (g2r_accum), to affine; set_ok = no selected
//                         key undecodable && sum != infinity (bls_verify_multisig_kernel's ok); or, for
//                         cbft_bls_sum_keys_batch, the compressed sum and ok of g2_sum_tail
//   blsm_lines_kernel     one wave per usable set: bls_keys_row_kernel's lines task on PK[j]
//                         (g2r_lines_abc, g2r_normalise_lines) into set_lines[j]
//   then the decode, hash and pairing kernels of bls_verify_batch.hip as they are, through
//   cbft_bls_verify_batch_launch: the sets are its key slots (key_idx = set_of, lines = set_lines,
//   key_ok = set_ok, slots 0 .. s - 1).
//
// Stream order is the only synchronisation between the stages: the lines are complete before the
// pairing launch starts.
#include "bls_multisig_batch.h"

#include "bls_common.h"
#include "bls_g2_shared.h"

static __host__ __device__ inline uint32_t blsm_chunks(uint32_t nkeys) {
  const uint32_t k = nkeys > 2048u ? 2048u : nkeys;  // the bitmap has 2,048 bits
  return k ? (k + BLS_MULTISIG_CHUNK - 1) / BLS_MULTISIG_CHUNK : 1u;
}
// per-set tables, in words after the verification's own scratch: lines | affine sums | partials | identity
// set_of | set_ok bytes
static inline size_t blsm_aff_at(size_t s) { return (size_t)LINES_PER_KEY * s; }
static inline size_t blsm_parts_at(size_t s) { return blsm_aff_at(s) + (size_t)BLS_G2A_WORDS * s; }
static inline size_t blsm_ident_at(size_t s, uint32_t nkeys) {
  return blsm_parts_at(s) + (size_t)BLS_G2_PART_WORDS * blsm_chunks(nkeys) * s;
}
static inline size_t blsm_tables_bytes(size_t n, size_t s, uint32_t nkeys) {
  return (blsm_ident_at(s, nkeys) + n) * sizeof(uint32_t) + s;
}
static inline size_t blsm_verify_bytes(size_t n, size_t m) {
  return (cbft_bls_verify_batch_scratch_bytes(n, m) + 15) & ~(size_t)15;
}
size_t cbft_bls_multisig_sum_scratch_bytes(size_t s, uint32_t nkeys) { return blsm_tables_bytes(0, s, nkeys); }
size_t cbft_bls_multisig_batch_scratch_bytes(size_t n, size_t m, size_t s, uint32_t nkeys) {
  return blsm_verify_bytes(n, m) + blsm_tables_bytes(n, s, nkeys);
}

// block b: chunk b % chunks of set b / chunks, ids [1 + 64 chunk, + 64) within [1, nkeys]
__global__ void __launch_bounds__(64) blsm_sum_part_kernel(const uint32_t* aff, const uint8_t* key_ok,
                                                           const uint8_t* signers, uint32_t nkeys, uint32_t chunks,
                                                           uint32_t s, uint32_t* parts) {
  const uint32_t j = blockIdx.x / chunks, ch = blockIdx.x - j * chunks;
  if (j >= s) return;
  const G2RCtx c(0u);
  G2R<uint32_t> acc{{c.one, c.zero}, {c.one, c.zero}, {c.zero, c.zero}};
  bool inf = true, bad = false;
  const uint8_t* bm = signers + 256 * (size_t)j + (BLS_MULTISIG_CHUNK / 8) * ch;
  const uint32_t id0 = 1 + BLS_MULTISIG_CHUNK * ch;
#pragma nounroll
  for (uint32_t q = 0; q < BLS_MULTISIG_CHUNK / 8; q++) {
    uint32_t bits = bm[q];  // wave-uniform
#pragma nounroll
    while (bits) {
      const uint32_t t = __builtin_ctz(bits);
      bits &= bits - 1;
      const uint32_t id = id0 + 8 * q + t;
      if (id > nkeys) break;  // bits above n_keys are ignored
      if (!key_ok[id]) {
        bad = true;
        continue;
      }
      const uint32_t* a = aff + (size_t)id * BLS_G2A_WORDS;  // x.a x.b y.a y.b (g2a_store)
      g2r_accum_aff(acc, inf, f2r_ld(a), f2r_ld(a + 18), c);
    }
  }
  g2r_part_store(parts + (size_t)BLS_G2_PART_WORDS * blockIdx.x, acc, inf, bad, c);
}

// block j: set j's partials -> its affine sum and set_ok (out65 == nullptr), or out65 / ok as
// cbft_bls_sum_keys writes them
__global__ void __launch_bounds__(64) blsm_sum_fin_kernel(const uint32_t* parts, uint32_t chunks, uint32_t s,
                                                          uint32_t* set_aff, uint8_t* set_ok, uint8_t* out65,
                                                          uint8_t* ok) {
  __shared__ uint32_t fin[BLS_G2_PART_WORDS];
  const uint32_t j = blockIdx.x;
  if (j >= s) return;
  const G2RCtx c(0u);
  G2R<uint32_t> acc{{c.one, c.zero}, {c.one, c.zero}, {c.zero, c.zero}};
  bool inf = true, bad = false;
#pragma nounroll
  for (uint32_t i = 0; i < chunks; i++) {
    const uint32_t* o = parts + (size_t)BLS_G2_PART_WORDS * ((size_t)j * chunks + i);
    G2R<uint32_t> q;
    const bool qinf = g2r_part_load(q, o, c);
    bad |= o[54] != 0;
    g2r_accum(acc, inf, q, qinf, c);
  }
  g2r_part_store(fin, acc, inf, bad, c);
  __syncthreads();  // one-wave block: lane 0 reads what lanes 0 .. 8 stored
  if (__lane_id() != 0) return;
  g2j sj;
  g2j_load(sj, fin);
  if (out65) {
    g2_sum_tail(sj, bad, ok + j, out65 + 65 * (size_t)j);
    return;
  }
  g2a a;
  g2_to_affine<true>(a, sj);  // public point: variable-time inversion
  set_ok[j] = !bad && !a.inf ? 1 : 0;
  g2a_store(set_aff + (size_t)BLS_G2A_WORDS * j, a);
}

// block j: the 70 normalised lines of PK[j], for the sets an item can pass the gate with
__global__ void __launch_bounds__(64) blsm_lines_kernel(const uint32_t* set_aff, const uint8_t* set_ok, uint32_t s,
                                                        uint32_t* set_lines) {
  __shared__ uint32_t abc[BN_ATE_LINES * BN_ABC_WORDS];
  __shared__ uint32_t pre[BN_ATE_LINES * 18];
  const uint32_t j = blockIdx.x;
  if (j >= s || !set_ok[j]) return;
  g2a q;
  g2a_load(q, set_aff + (size_t)BLS_G2A_WORDS * j);
  g2r_lines_abc(abc, q);
  g2r_normalise_lines(set_lines + (size_t)j * LINES_PER_KEY, abc, pre);
}

// set_of == nullptr: item i uses set i (the verification's own nullptr means slot 0)
__global__ void __launch_bounds__(256) blsm_ident_kernel(uint32_t* ident, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) ident[i] = i;
}

static hipError_t blsm_sum(const BlsMultisigBatch& b, uint32_t* t, uint8_t* d_out65, uint8_t* d_ok, hipStream_t st) {
  const uint32_t chunks = blsm_chunks(b.nkeys);
  uint32_t* parts = t + blsm_parts_at(b.s);
  hipLaunchKernelGGL(blsm_sum_part_kernel, dim3(b.s * chunks), dim3(64), 0, st, b.aff, b.key_ok, b.signers, b.nkeys,
                     chunks, b.s, parts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  uint8_t* set_ok = reinterpret_cast<uint8_t*>(t + blsm_ident_at(b.s, b.nkeys) + b.n);
  hipLaunchKernelGGL(blsm_sum_fin_kernel, dim3(b.s), dim3(64), 0, st, (const uint32_t*)parts, chunks, b.s,
                     t + blsm_aff_at(b.s), set_ok, d_out65, d_ok);
  return hipGetLastError();
}

hipError_t cbft_bls_multisig_sum_launch(const BlsMultisigBatch& b, void* d_scratch, uint8_t* d_out65, uint8_t* d_ok,
                                        hipStream_t st) {
  if (!b.s) return hipSuccess;
  if (b.s > BLS_MULTISIG_MAX_SETS || b.n) return hipErrorInvalidValue;  // the sum-only layout has no items
  return blsm_sum(b, static_cast<uint32_t*>(d_scratch), d_out65, d_ok, st);
}

hipError_t cbft_bls_multisig_batch_launch(const BlsMultisigBatch& b, void* d_scratch, uint8_t* d_valid, hipStream_t st) {
  if (!b.n) return hipSuccess;
  if (!b.s) return hipMemsetAsync(d_valid, 0, b.n, st);  // no set is in range
  if (b.s > BLS_MULTISIG_MAX_SETS) return hipErrorInvalidValue;
  uint32_t* t = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(d_scratch) + blsm_verify_bytes(b.n, b.m));
  uint32_t* set_lines = t;
  uint32_t* ident = t + blsm_ident_at(b.s, b.nkeys);
  uint8_t* set_ok = reinterpret_cast<uint8_t*>(ident + b.n);
  hipError_t e = blsm_sum(b, t, nullptr, nullptr, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(blsm_lines_kernel, dim3(b.s), dim3(64), 0, st, (const uint32_t*)(t + blsm_aff_at(b.s)),
                     (const uint8_t*)set_ok, b.s, set_lines);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (!b.set_of) {
    hipLaunchKernelGGL(blsm_ident_kernel, dim3((b.n + 255) / 256), dim3(256), 0, st, ident, b.n);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  BlsVerifyBatch v{};
  v.n = b.n;
  v.m = b.m;
  v.key_idx = b.set_of ? b.set_of : ident;
  v.msg_of = b.msg_of;
  v.sig33 = b.sig33;
  v.msg = b.msg;
  v.off = b.off;
  v.len = b.len;
  v.fixed_len = b.fixed_len;
  v.nkeys = b.s - 1;  // slots 0 .. s - 1
  v.lines = set_lines;
  v.key_ok = set_ok;
  v.gen_lines = b.gen_lines;
  return cbft_bls_verify_batch_launch(v, d_scratch, d_valid, st);
}
