// k_ecdsa_verify: one lane per record of the ECDSA P-256 batch verifier
// (include/cess_ecdsa.h; arithmetic and rules in p256.hpp).
//
// Per record: KEY for an index outside the table or a key that did not load,
// then k_ecdsa_pack's code (SIG_FORMAT, SIG_RANGE); e from the leftmost 32
// bytes of the record's digest (k_rsa_digest or k_rsa_digest512 over
// k_ecdsa_pack's buffer), minus n once; w = 1 / s by the fixed chain, u1 = e w,
// u2 = r w, both recoded to 65 signed radix-16 digits; one ladder of 64 rounds
// of four doublings, an addition from table[key][|digit of u2|] and one from
// table_g[|digit of u1|]; then ring's test r Z^2 = X, and (r + n) Z^2 = X where
// r < q - n (p256::verify_scalars).  No field inversion per record.
//
// A zero digit adds nothing and equal or opposite operands take their own
// branch: the lanes of a wave diverge there (one digit in 16 is zero).  A
// record that already has a code stores it and leaves, so no lane ever reads a
// row of a key that did not load or of an index outside the table, and a batch
// of invalid records costs what its valid lanes cost.  Lanes past n leave at
// once.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "p256.hpp"

__global__ CESS_LB void k_ecdsa_verify(uint64_t n, const uint32_t* __restrict__ key_idx, uint32_t nkeys,
                                       const uint8_t* __restrict__ status, const uint32_t* __restrict__ table,
                                       const uint32_t* __restrict__ table_g, const uint32_t* __restrict__ rec,
                                       const uint8_t* __restrict__ digests, uint32_t digest_stride,
                                       uint8_t* __restrict__ codes) {
  using namespace p256;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t idx = key_idx[i];
  const bool key_ok = idx < nkeys && status[idx < nkeys ? idx : 0] == KEY_LOADED;
  const uint32_t* o = rec + (uint64_t)kRecWords * i;
  const uint32_t early = key_ok ? o[16] : (uint32_t)EC_KEY;
  if (early != EC_OK) {
    codes[i] = (uint8_t)early;
    return;
  }
  uint32_t e[8], r[8], s[8];
  digest_scalar(digests + (uint64_t)digest_stride * i, e);
#pragma unroll
  for (int q = 0; q < 8; q++) r[q] = o[q], s[q] = o[8 + q];
  const bool ok = verify_scalars(table + (uint64_t)kTableWords * idx, table_g, e, r, s);
  codes[i] = (uint8_t)(ok ? EC_OK : EC_MISMATCH);
}
