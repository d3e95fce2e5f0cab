// k_ecdsa_keys and k_ecdsa_pack: the per-key and per-record front ends of the
// ECDSA P-256 batch verifier (include/cess_ecdsa.h; arithmetic and rules in
// p256.hpp).  One lane per key / per record.
//
// k_ecdsa_keys.  Key j of the caller's offset-indexed bytes: rule 1 (65 bytes,
// 0x04, x and y below q, on the curve) and the signed-window table of Q -- the
// multiples 1..8 as affine Montgomery digits, normalised with one shared
// inversion (p256::key_table) -- into table[j] (960 bytes) and the status into
// status[j].  The context's table of G is this kernel's output for G's
// encoding.  The table lives in HBM because it is read-only and shared by all
// records of a key.
//
// k_ecdsa_pack.  Record i's signature is split (FIXED) or parsed (ASN.1, ring's
// der.rs) into r and s, checked against [1, n - 1], and written with its early
// code (OK, SIG_FORMAT, SIG_RANGE) as 17 words to rec[i]; r and s are zero
// where the code is not OK.  Its message goes to pack[po[i]], po[i] =
// msg_offs[i] - msg_offs[0], the layout the digest kernels take (prefix = 0).
// A record whose message offsets are not ordered inside [msg_offs[0],
// msg_offs[n]] copies no bytes, and one whose signature offsets are not ordered
// inside [sig_offs[0], sig_offs[n]] is an empty signature, so every load and
// store lies inside the ranges the offsets' ends give.
#include <hip/hip_runtime.h>

#include "p256.hpp"

// (one wave per SIMD: the seven prefix products of pass 1 stay in registers)
__global__ __launch_bounds__(64, 1) void k_ecdsa_keys(uint64_t k, const uint8_t* __restrict__ keys,
                                                      const uint64_t* __restrict__ offs, uint32_t* table,
                                                      uint8_t* __restrict__ status) {
  const uint64_t j = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (j >= k) return;
  const uint64_t b = offs[j], len = offs[j + 1] - b;
  status[j] = p256::key_table(keys + b, len, table + (uint64_t)p256::kTableWords * j);
}

__global__ __launch_bounds__(256) void k_ecdsa_pack(uint64_t n, uint32_t alg, const uint8_t* __restrict__ sigs,
                                                    const uint64_t* __restrict__ sig_offs,
                                                    const uint8_t* __restrict__ msgs,
                                                    const uint64_t* __restrict__ msg_offs, uint8_t* __restrict__ pack,
                                                    uint64_t* __restrict__ po, uint32_t* __restrict__ rec) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  const uint64_t m0 = msg_offs[0], mn = msg_offs[n], mb = msg_offs[i];
  const bool b_ok = m0 <= mb && mb <= mn;
  const uint64_t at = b_ok ? mb - m0 : 0;
  po[i] = at;
  if (i == n) return;
  const uint64_t me = msg_offs[i + 1];
  const uint64_t len = b_ok && mb <= me && me <= mn ? me - mb : 0;
  uint8_t* out = pack + at;
#pragma unroll 1
  for (uint64_t q = 0; q < len; q++) out[q] = msgs[mb + q];
  const uint64_t s0 = sig_offs[0], sn = sig_offs[n], sb = sig_offs[i], se = sig_offs[i + 1];
  const bool s_ok = s0 <= sb && sb <= se && se <= sn;
  uint32_t r[8], s[8];
  const uint32_t code = p256::parse_sig(alg, sigs + (s_ok ? sb : s0), s_ok ? se - sb : 0, r, s);
  uint32_t* o = rec + (uint64_t)p256::kRecWords * i;
#pragma unroll
  for (int q = 0; q < 8; q++) {
    o[q] = code == p256::EC_OK ? r[q] : 0u;
    o[8 + q] = code == p256::EC_OK ? s[q] : 0u;
  }
  o[16] = code;
}
