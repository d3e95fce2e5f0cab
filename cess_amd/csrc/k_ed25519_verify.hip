// k_ed25519_verify: one lane per record of the Ed25519 batch verifier
// (include/cess_ed25519.h; arithmetic and rules in ed25519.hpp).
//
// Per record: the codes 1..3 first (ed25519::early_code, in the header's
// order); h = the record's SHA-512 digest (k_rsa_digest512 over
// k_ed25519_pack's buffer) as a little-endian integer reduced mod L; S and h
// recoded to 64 signed radix-16 digits; then 64 rounds of four doublings, one
// mixed addition from table[key][|digit of h|] (the multiples of -A) and one
// from table_b[|digit of S|] (those of B), one inversion, the canonical
// encoding and the 32-byte compare with R (ed25519::verify_equation).  R is
// never decoded.
//
// Control flow is wave-uniform: a zero digit selects the identity entry (the
// row of multiple 1 is read and replaced; the addition still runs), a sign is a
// swap and a negation of the entry, and a record that already has a code runs
// the same rounds on zero scalars with table_b in place of its key's table, so
// no lane ever reads a row of a key that did not load or of an index outside
// the table.  Lanes past n leave at once.
//
// Registers: the point (4 field elements), the four factors of a doubling or
// addition (4), the entry (3) and the two recoded scalars: under the 256 VGPRs
// of two waves per SIMD, no scratch (tests/test_ed25519.py reads the notes).
#include <hip/hip_runtime.h>

#include "ed25519.hpp"
#include "kernels.hpp"

__global__ CESS_LB void k_ed25519_verify(uint64_t n, const uint32_t* __restrict__ key_idx, uint32_t nkeys,
                                         const uint8_t* __restrict__ status, const uint32_t* __restrict__ table,
                                         const uint32_t* __restrict__ table_b, const uint8_t* __restrict__ sigs,
                                         const uint64_t* __restrict__ sig_offs, const uint8_t* __restrict__ digests,
                                         uint8_t* __restrict__ codes) {
  using namespace ed25519;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t idx = key_idx[i];
  const uint8_t st = idx < nkeys ? status[idx] : (uint8_t)KEY_BAD_LEN;
  const uint64_t sb = sig_offs[i], slen = sig_offs[i + 1] - sb;
  uint32_t R[8], S[8], h[8];
#pragma unroll
  for (int q = 0; q < 8; q++) R[q] = S[q] = 0;
  if (slen == 64) {
    load_words(sigs + sb, R);
    load_words(sigs + sb + 32, S);
  }
  const uint32_t early = early_code(st, slen, S);
  const bool active = early == ED_OK;
  {
    uint32_t x[16];
    const uint32_t* d = reinterpret_cast<const uint32_t*>(digests + 64 * i);
#pragma unroll
    for (int q = 0; q < 16; q++) x[q] = d[q];
    sc_reduce512(x, h);
  }
#pragma unroll
  for (int q = 0; q < 8; q++) {
    S[q] = active ? S[q] : 0u;
    h[q] = active ? h[q] : 0u;
  }
  const uint32_t* tab_a = active ? table + (uint64_t)kTableWords * idx : table_b;
  const bool ok = verify_equation(tab_a, table_b, S, h, R);
  codes[i] = (uint8_t)(active ? (ok ? ED_OK : ED_MISMATCH) : early);
}
