// The kernels of the Ed25519 batch signer (include/cess_ed25519_sign.h;
// arithmetic and rules in ed25519_sign.hpp over ed25519.hpp).  One lane per
// table row, signer or record.
//
// k_ed25519_comb.  Once per context: lane i of one 64-lane block builds row i of
// the comb table, the multiples 1..8 of 16^i B (ed25519::comb_row), into
// comb[i] (960 bytes) and its status into status[i].  The table lives in HBM and
// is read through cache, like the key tables of the verifier.
//
// k_ed25519_signers.  Signer j from the SHA-512 digest of its seed
// (k_rsa_digest512 over the staged seeds): clamp, a mod L, A = encode([a]B), the
// compare with expected[j] (32 bytes each, or null).  It stores a mod L, the
// prefix and A for a signer that loaded; zeros in a and prefix otherwise (and in
// A for a seed that is not 32 bytes), so no record can sign with them.
//
// k_ed25519_sign_pack.  Record i's hash input at pack[po[i]], the layout
// k_rsa_digest512 takes (prefix = 0, SHA-512).  With sigs == null it is
// head[signer] || msg (the nonce input, head = the signers' prefixes) and
// po[i] = 32 i + (msg_offs[i] - msg_offs[0]); otherwise sigs[64 i .. 64 i + 32) ||
// head[signer] || msg (head = the signers' A) and po[i] = 64 i + ....  A record
// whose signer is missing or did not load takes zeros for head; one whose
// message offsets are not ordered inside [msg_offs[0], msg_offs[n]] copies no
// message bytes, so every store lies inside the H n + (msg_offs[n] -
// msg_offs[0]) bytes of the buffer.
//
// k_ed25519_sign_r.  r = digest mod L, R = encode([r]B) into sigs[64 i ..
// 64 i + 32), r into nonces[i].  k_ed25519_sign_s.  k = digest mod L, S = (k a +
// r) mod L into sigs[64 i + 32 .. 64 i + 64) and the record's code.  A record
// whose signer is missing runs the same code on zero scalars and gets 64 zero
// bytes and CESS_ED25519_SIGN_SIGNER; no lane reads a row outside the table.
//
// Registers of k_ed25519_sign_r: the point (4 field elements), the four factors
// of an addition, the entry (3) and one recoded scalar: under the 256 VGPRs of
// two waves per SIMD, no scratch (tests/test_ed25519_sign.py reads the notes).
#include <hip/hip_runtime.h>

#include "ed25519_sign.hpp"
#include "kernels.hpp"

using namespace ed25519;

// (one wave per SIMD, as k_ed25519_keys: key_table's prefix products stay in registers)
__global__ __launch_bounds__(64, 1) void k_ed25519_comb(uint32_t* comb, uint8_t* __restrict__ status) {
  const int i = threadIdx.x;
  if (blockIdx.x != 0 || i >= kCombRows) return;
  status[i] = comb_row(i, comb + (uint64_t)kTableWords * i);
}

__global__ CESS_LB void k_ed25519_signers(uint64_t k, const uint32_t* __restrict__ comb,
                                          const uint64_t* __restrict__ offs, const uint8_t* __restrict__ digests,
                                          const uint8_t* __restrict__ expected, uint32_t* __restrict__ a_out,
                                          uint32_t* __restrict__ prefix, uint32_t* __restrict__ pubs,
                                          uint8_t* __restrict__ status) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const bool len_ok = offs[j + 1] - offs[j] == 32;
  uint32_t h[16], a[8], A[8];
  load_digest(digests + 64 * j, h);
  const uint8_t st = signer_derive(comb, h, len_ok, expected ? expected + 32 * j : nullptr, a, A);
#pragma unroll
  for (int q = 0; q < 8; q++) {
    a_out[8 * j + q] = st == SIGNER_LOADED ? a[q] : 0u;
    prefix[8 * j + q] = st == SIGNER_LOADED ? h[8 + q] : 0u;
    pubs[8 * j + q] = len_ok ? A[q] : 0u;
  }
  status[j] = st;
}

__global__ __launch_bounds__(256) void k_ed25519_sign_pack(uint64_t n, const uint32_t* __restrict__ signer_idx,
                                                           uint32_t nsigners, const uint8_t* __restrict__ status,
                                                           const uint8_t* __restrict__ head, const uint8_t* sigs,
                                                           const uint8_t* __restrict__ msgs,
                                                           const uint64_t* __restrict__ msg_offs,
                                                           uint8_t* __restrict__ pack, uint64_t* __restrict__ po) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  const uint64_t m0 = msg_offs[0], mn = msg_offs[n], mb = msg_offs[i];
  const bool b_ok = m0 <= mb && mb <= mn;
  const uint64_t at = (sigs ? 64 : 32) * i + (b_ok ? mb - m0 : 0);
  po[i] = at;
  if (i == n) return;
  const uint64_t me = msg_offs[i + 1];
  const uint64_t len = b_ok && mb <= me && me <= mn ? me - mb : 0;
  const uint32_t idx = signer_idx[i];
  const bool ok = idx < nsigners && status[idx < nsigners ? idx : 0] == SIGNER_LOADED;
  uint8_t* out = pack + at;
  if (sigs) {
#pragma unroll 1
    for (int q = 0; q < 32; q++) out[q] = sigs[64 * i + q];
    out += 32;
  }
#pragma unroll 1
  for (int q = 0; q < 32; q++) out[q] = ok ? head[32ull * idx + q] : (uint8_t)0;
#pragma unroll 1
  for (uint64_t q = 0; q < len; q++) out[32 + q] = msgs[mb + q];
}

__global__ CESS_LB void k_ed25519_sign_r(uint64_t n, const uint32_t* __restrict__ signer_idx, uint32_t nsigners,
                                         const uint8_t* __restrict__ status, const uint32_t* __restrict__ comb,
                                         const uint8_t* __restrict__ digests, uint32_t* __restrict__ nonces,
                                         uint8_t* __restrict__ sigs) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t idx = signer_idx[i];
  const bool ok = idx < nsigners && status[idx < nsigners ? idx : 0] == SIGNER_LOADED;
  uint32_t x[16], r[8], R[8];
  load_digest(digests + 64 * i, x);
  sc_reduce512(x, r);
#pragma unroll
  for (int q = 0; q < 8; q++) r[q] = ok ? r[q] : 0u;
  ge_scalarmult_base(comb, r, R);
#pragma unroll
  for (int q = 0; q < 8; q++) {
    nonces[8 * i + q] = r[q];
    R[q] = ok ? R[q] : 0u;
  }
  store_bytes32(sigs + 64 * i, R);
}

__global__ CESS_LB void k_ed25519_sign_s(uint64_t n, const uint32_t* __restrict__ signer_idx, uint32_t nsigners,
                                         const uint8_t* __restrict__ status, const uint32_t* __restrict__ a_tab,
                                         const uint8_t* __restrict__ digests, const uint32_t* __restrict__ nonces,
                                         uint8_t* __restrict__ sigs, uint8_t* __restrict__ codes) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t idx = signer_idx[i];
  const bool ok = idx < nsigners && status[idx < nsigners ? idx : 0] == SIGNER_LOADED;
  uint32_t x[16], k[8], a[8], r[8], S[8];
  load_digest(digests + 64 * i, x);
  sc_reduce512(x, k);
#pragma unroll
  for (int q = 0; q < 8; q++) {
    a[q] = a_tab[8ull * (ok ? idx : 0u) + q];
    r[q] = nonces[8 * i + q];
  }
  sc_muladd(k, a, r, S);
#pragma unroll
  for (int q = 0; q < 8; q++) S[q] = ok ? S[q] : 0u;
  store_bytes32(sigs + 64 * i + 32, S);
  if (codes) codes[i] = (uint8_t)(ok ? SIGN_OK : SIGN_SIGNER);
}
