// k_ed25519_keys and k_ed25519_pack: the per-key and per-record front ends of
// the Ed25519 batch verifier (include/cess_ed25519.h; arithmetic and rules in
// ed25519.hpp).  One lane per key / per record.
//
// k_ed25519_keys.  Key j of the caller's offset-indexed bytes: length check,
// decoding (rule 4), and the signed-window table of -A -- the multiples 1..8 as
// affine entries (y + x, y - x, 2 d x y), normalised with one shared inversion
// (ed25519::key_table) -- into table[j] (960 bytes), the status into status[j]
// and the 32 key bytes as given (zeros for another length) into raw[j], which
// k_ed25519_pack puts into the hash input.  The context's table of the base
// point is this kernel's output for the encoding of -B.  The table lives in HBM
// because it is read-only and shared by all records of a key: a batch under few
// keys (the TEE workload) reads it from cache, and no lane keeps a table in
// VGPRs, LDS or scratch.
//
// k_ed25519_pack.  Record i's hash input R || key || msg at pack[po[i]] with
// po[i] = 64 i + (msg_offs[i] - msg_offs[0]), the layout k_rsa_digest512 takes
// (prefix = 0, SHA-512).  R is sig[0..32) where the signature has 64 bytes and
// the key bytes are raw[key_idx[i]] where the index is in the table, zeros
// otherwise (such records have a code already; their digest is not used).  A
// record whose message offsets are not ordered inside [msg_offs[0],
// msg_offs[n]] copies no message bytes, so every store lies inside the
// 64 n + (msg_offs[n] - msg_offs[0]) bytes of the buffer.
#include <hip/hip_runtime.h>

#include "ed25519.hpp"

// (one wave per SIMD: the seven prefix products of pass 1 stay in registers)
__global__ __launch_bounds__(64, 1) void k_ed25519_keys(uint64_t k, const uint8_t* __restrict__ keys,
                                                        const uint64_t* __restrict__ offs, uint32_t* table,
                                                        uint8_t* __restrict__ status, uint8_t* __restrict__ raw) {
  const uint64_t j = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (j >= k) return;
  const uint64_t b = offs[j], len = offs[j + 1] - b;
  status[j] = ed25519::key_table(keys + b, len, table + (uint64_t)ed25519::kTableWords * j);
#pragma unroll 1
  for (int q = 0; q < 32; q++) raw[32 * j + q] = len == 32 ? keys[b + q] : (uint8_t)0;
}

__global__ __launch_bounds__(256) void k_ed25519_pack(uint64_t n, const uint32_t* __restrict__ key_idx, uint32_t nkeys,
                                                      const uint8_t* __restrict__ raw, const uint8_t* __restrict__ sigs,
                                                      const uint64_t* __restrict__ sig_offs,
                                                      const uint8_t* __restrict__ msgs,
                                                      const uint64_t* __restrict__ msg_offs, uint8_t* __restrict__ pack,
                                                      uint64_t* __restrict__ po) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  const uint64_t m0 = msg_offs[0], mn = msg_offs[n], mb = msg_offs[i];
  const bool b_ok = m0 <= mb && mb <= mn;
  const uint64_t at = 64 * i + (b_ok ? mb - m0 : 0);
  po[i] = at;
  if (i == n) return;
  const uint64_t me = msg_offs[i + 1];
  const uint64_t len = b_ok && mb <= me && me <= mn ? me - mb : 0;
  const uint64_t sb = sig_offs[i], slen = sig_offs[i + 1] - sb;
  const uint32_t idx = key_idx[i];
  uint8_t* out = pack + at;
#pragma unroll 1
  for (int q = 0; q < 32; q++) out[q] = slen == 64 ? sigs[sb + q] : (uint8_t)0;
#pragma unroll 1
  for (int q = 0; q < 32; q++) out[32 + q] = idx < nkeys ? raw[32ull * idx + q] : (uint8_t)0;
#pragma unroll 1
  for (uint64_t q = 0; q < len; q++) out[64 + q] = msgs[mb + q];
}
