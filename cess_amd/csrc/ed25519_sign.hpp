// Ed25519 key derivation and signing under ring's rules
// (include/cess_ed25519_sign.h): what k_ed25519_sign.hip and the host build of
// the same code (tests/hostemu/ed25519_sign_emu.cpp, -DCESS_HOSTEMU) add to
// ed25519.hpp, which is included unchanged.  The rules are read from ring's
// ed25519/signing.rs (Ed25519KeyPair::from_seed_unchecked,
// from_seed_and_public_key, sign); the code is this project's.
//
// Fixed-base multiplication.  [s]B for s < L is the sum over the 64 signed
// radix-16 digits d_i of s (sc_recode) of d_i * 16^i * B.  The comb table holds,
// for every position i, the eight multiples j * 16^i * B (j = 1..8) as affine
// entries (y + x, y - x, 2 d x y): 64 rows of 960 bytes, 61,440 bytes, built once
// per context by the code that builds a key's table (key_table on the encoding
// of -(16^i B), which negates again).  One mixed addition per digit and no
// doubling: 64 x 7 = 448 multiplies, then the inversion (254 squarings, 11
// multiplies) and the canonical encoding, as verify_equation ends.  Rows are
// addressed by the digits of a secret scalar: the code is wave-uniform in its
// control flow, but NOT constant-time in its memory accesses.
//
// a mod L.  sc_recode is exact only while s + 0x88..8 < 2^256, that is for
// s < 2^256 * 7 / 15.  A clamped scalar a lies in [2^254, 2^255) and exceeds that
// bound when its top bits are high (about 9 seeds in 64): the carry out of the
// top word would be lost and the digits would be those of a - 2^256.  B has
// order L, so [a]B = [a mod L]B: signer_derive reduces a once, the table keeps
// a mod L, and sc_muladd(k, a mod L, r) is the same S = (k a + r) mod L.
#pragma once
#include "ed25519.hpp"

namespace ed25519 {

constexpr int kCombRows = 64;                          // one per radix-16 digit of a scalar below 2^256
constexpr int kCombWords = kCombRows * kTableWords;    // 61,440 bytes

// per-signer status of the table: loaded; the seed is not 32 bytes; the
// expected public key differs from the derived one
enum : uint8_t { SIGNER_LOADED = 0, SIGNER_BAD_LEN = 1, SIGNER_INCONSISTENT = 2 };
enum : uint32_t { SIGN_OK = 0, SIGN_SIGNER = 1 };

// RFC 8032 5.1.5 step 2 on the low half of SHA-512(seed): bits 0, 1, 2 and 255
// cleared, bit 254 set
CESS_HD void clamp(uint32_t (&a)[8]) {
  a[0] &= 0xfffffff8u;
  a[7] = (a[7] & 0x7fffffffu) | 0x40000000u;
}

// a mod L for a 256-bit a
CESS_HD void sc_reduce256(const uint32_t (&a)[8], uint32_t (&out)[8]) {
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 16; i++) x[i] = i < 8 ? a[i] : 0u;
  sc_reduce512(x, out);
}

// (k a + r) mod L for any 256-bit k, a and r: the product and the sum stay below 2^512
CESS_HD void sc_muladd(const uint32_t (&k)[8], const uint32_t (&a)[8], const uint32_t (&r)[8], uint32_t (&out)[8]) {
  uint32_t x[16], carry = 0;
  sc_mul<8, 8>(k, a, x);
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const uint64_t t = (uint64_t)x[i] + (i < 8 ? r[i] : 0u) + carry;
    x[i] = (uint32_t)t;
    carry = (uint32_t)(t >> 32);
  }
  sc_reduce512(x, out);
}

// the canonical 32 bytes of a point, as 8 words: one inversion
CESS_HD void ge_encode(const ge_p3& p, uint32_t (&w)[8]) {
  const fe zi = fe_invert(p.Z);
  const fe x = fe_mul(p.X, zi), y = fe_mul(p.Y, zi);
  fe_to_words(y, w);
  w[7] |= fe_is_negative(x) << 31;
}

// encode([s]B) for s < L from the comb table: the digits are read from the low
// nibble of the recoded scalar, which shifts right by 4 per round, so no word is
// indexed by the loop counter; every lane runs all 64 additions (a zero digit
// adds the identity entry)
CESS_HD void ge_scalarmult_base(const uint32_t* comb, const uint32_t (&s)[8], uint32_t (&enc)[8]) {
  uint32_t r[8];
  sc_recode(s, r);
  ge_p3 p = {fe_small(0), fe_small(1), fe_small(1), fe_small(0)};
#pragma unroll 1
  for (int i = 0; i < kCombRows; i++) {
    const int d = (int)(r[0] & 15u) - 8;
#pragma unroll
    for (int q = 0; q < 7; q++) r[q] = (r[q] >> 4) | (r[q + 1] << 28);
    r[7] >>= 4;
    const ge_pre e = ge_pre_digit(comb + (uint64_t)kTableWords * i, d);
    fe E, H, G, F;
    ge_madd(p, e, E, H, G, F);
    ge_finish(p, E, H, G, F, true);
  }
  ge_encode(p, enc);
}

// Row i of the comb table: the multiples 1..8 of 16^i B.  B is decoded from the
// encoding of -B and doubled 4 i times (every lane runs all 252 doublings and
// keeps the first 4 i of them), normalised, and -(16^i B) is encoded for
// key_table, which builds the table of the negated point.  `row`: kTableWords
// words, this row's alone.  Returns key_table's status (KEY_LOADED).
CESS_HD uint8_t comb_row(int i, uint32_t* row) {
  uint32_t w[8];
#pragma unroll
  for (int q = 0; q < 8; q++)
    w[q] = (uint32_t)kNegBaseEnc[4 * q] | ((uint32_t)kNegBaseEnc[4 * q + 1] << 8) |
           ((uint32_t)kNegBaseEnc[4 * q + 2] << 16) | ((uint32_t)kNegBaseEnc[4 * q + 3] << 24);
  fe x, y;
  const bool ok = ge_decode(w, x, y);
  ge_p3 p = {fe_neg(x), y, fe_small(1), fe_small(0)};   // B (doubling reads no T)
#pragma unroll 1
  for (int j = 0; j < 4 * (kCombRows - 1); j++) {
    ge_p3 q = p;
    fe E, H, G, F;
    ge_dbl(p, E, H, G, F);
    ge_finish(q, E, H, G, F, false);
    const bool keep = j < 4 * i;
    p.X = fe_select(keep, q.X, p.X);
    p.Y = fe_select(keep, q.Y, p.Y);
    p.Z = fe_select(keep, q.Z, p.Z);
  }
  const fe zi = fe_invert(p.Z);
  const fe ax = fe_mul(p.X, zi), ay = fe_mul(p.Y, zi);
  fe_to_words(ay, w);
  w[7] |= fe_is_negative(fe_neg(ax)) << 31;              // the sign of -x
  uint8_t enc[32];
#pragma unroll
  for (int q = 0; q < 32; q++) enc[q] = (uint8_t)(w[q >> 2] >> (8 * (q & 3)));
  const uint8_t st = key_table(enc, 32, row);
  return ok ? st : (uint8_t)KEY_BAD_POINT;
}

// One signer from h = SHA-512(seed) as 16 little-endian words: a = clamp(h[0..8))
// reduced mod L (see the head of this file), A = encode([a]B), and the compare
// with the caller's expected key (32 bytes, or null).  A seed of another length
// computes on a zero scalar.  The caller stores a and the prefix h[8..16) only
// for a signer that loaded.
CESS_HD uint8_t signer_derive(const uint32_t* comb, const uint32_t (&h)[16], bool len_ok, const uint8_t* expected,
                              uint32_t (&a)[8], uint32_t (&A)[8]) {
  uint32_t c[8];
#pragma unroll
  for (int i = 0; i < 8; i++) c[i] = h[i];
  clamp(c);
  sc_reduce256(c, a);
#pragma unroll
  for (int i = 0; i < 8; i++) a[i] = len_ok ? a[i] : 0u;
  ge_scalarmult_base(comb, a, A);
  uint32_t diff = 0;
  if (expected) {
    uint32_t e[8];
    load_words(expected, e);
#pragma unroll
    for (int i = 0; i < 8; i++) diff |= e[i] ^ A[i];
  }
  return !len_ok ? SIGNER_BAD_LEN : diff ? SIGNER_INCONSISTENT : SIGNER_LOADED;
}

// 16 little-endian words of a 64-byte digest at a 4-byte aligned address
CESS_HD void load_digest(const uint8_t* d, uint32_t (&x)[16]) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(d);
#pragma unroll
  for (int q = 0; q < 16; q++) x[q] = w[q];
}

CESS_HD void store_bytes32(uint8_t* out, const uint32_t (&w)[8]) {
#pragma unroll
  for (int q = 0; q < 32; q++) out[q] = (uint8_t)(w[q >> 2] >> (8 * (q & 3)));
}

}  // namespace ed25519
