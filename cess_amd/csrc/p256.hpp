// ECDSA P-256 verification under ring 0.16.9's rules (include/cess_ecdsa.h):
// the field mod q, scalars mod n, the curve and the signature parser, for
// k_ecdsa_keys.hip, k_ecdsa_verify.hip and the host build of the same code
// (tests/hostemu/ecdsa_emu.cpp, -DCESS_HOSTEMU).  The rules are read from
// ring's ec/suite_b/ecdsa/verification.rs, digest_scalar.rs, public_key.rs and
// io/der.rs; the code is this project's.
//
// Representation.  Field elements and scalars are ten 28-bit digits (digit k
// has weight 2^(28 k)) in Montgomery form with R = 2^280.  One digit product is
// one 32 x 32 + 64 multiply-add (v_mad_u64_u32) into a lazy 64-bit column, as
// in bls/field.hpp.  Why Montgomery and not a Solinas fold of a plain product:
// q = -1 (mod 2^96), so with 28-bit digits -1/q = 1 (mod 2^28) and the quotient
// digit of a column is the accumulator's low digit, with no multiply; three of
// q's ten digits are zero and their products are not issued.  A multiply mod q
// is 100 + 10 * 7 = 170 multiply-adds, a square 55 + 70 = 125, and the carry of
// a column is the shift the column needs anyway.  A Solinas fold keeps the
// 100 / 55 products but pays about 9 signed 32-bit word sums of 256-bit values
// per reduction, on 32-bit words that must first be rebuilt from 19 lazy
// 28-bit columns: more VALU instructions than the 70 multiply-adds it saves,
// and a second representation beside the scalars'.  n has no structure:
// scalars use the same template with all ten digits of n and the multiply by
// -1/n (200 and 155 multiply-adds).
//
// Bounds.  "tight": digits 0..8 below 2^28, digit 9 below 32, value below twice
// the modulus; what mul, sqr, fe_sub, fe_mulk and fe_canon return.  "lazy": a
// sum of at most three tight values, digits below 3 * 2^28 < 2^30; what fe_add
// returns.  mul and sqr take digits below 2^30 and values below 2^267 (a b <
// 2^534 < q R, so the result is below 2 q).  A column sums at most 10 operand
// products below 2^60 (a square: 5 below 2^61 and one below 2^60), at most 10
// reduction products below 2^56 and a carry below 2^37: below 11 * 2^60 + 2^37
// < 2^63.5 = kColBound.  The host build shadows every column in 128 bits and
// records the maximum (emu_ecdsa_col_max).  fe_sub(a, b) is a + 32 q - b for b
// below 32 q, carried with signed 32-bit digits (|a_i - b_i + (32 q)_i + carry|
// < 2^31), then brought below 2^256 + 2^230 by subtracting floor(v / 2^256) q,
// which is a second carry pass with five adjusted digits.  fe_mulk(a, k),
// k <= 8, does the same from k a.
//
// s^-1 mod n.  Fermat with a fixed chain for n - 2: 255 squarings and 80
// multiplies, 255 * 155 + 80 * 200 = 55.5 K multiply-adds, 10 % of a record
// (DESIGN.md §4).  The divstep inversion of bls/field.hpp issues no
// multiply-adds, but it is written for twelve 32-bit words and the 381-bit
// prime and runs 6 x 62 steps of 64-bit shifts and selects, which are two
// instructions each on this machine; the chain shares the multiply below and
// was taken.
//
// Curve.  Jacobian coordinates, a = -3, Z = 0 for infinity.  Doubling is
// dbl-2001-b (3 M + 5 S), the mixed addition 8 M + 3 S with explicit handling:
// an infinite first operand returns the affine one; H = 0 (equal x) doubles
// where the y agree and returns infinity where they do not.  The tests cost
// two compares of ten digits per addition (fe_is_zero on a tight value: all
// digits 0 or all equal q's) against about 11 multiplies of the addition
// itself; complete formulas (Renes-Costello-Batina, 11 M + 6 mults by
// constants mixed) would cost three to four multiplies more on every
// addition.  Nothing here is secret: the branches diverge on crafted inputs
// only -- which whoever picks the key Q = d G can craft, for any round and
// either addition (tests/ecdsa_ladder_model.py; DESIGN.md §4 says where each
// case is tested).  Table entries can not be infinite (n is prime and far
// above 8).
//
// Double multiplication: signed radix-16 digits of u1 and u2 (65 digits, the
// top one 0 or 1), one ladder of 64 rounds of four doublings sharing both
// scalars, two tables of the multiples 1..8, affine: G's once per context,
// the key's at keys_load, both built by key_table with one inversion.
#pragma once
#include <stdint.h>

#include "bls/field.hpp"   // CESS_HD, CESS_CONST

namespace p256 {

enum : uint32_t { EC_OK = 0, EC_SIG_FORMAT = 1, EC_SIG_RANGE = 2, EC_KEY = 3, EC_MISMATCH = 4 };
enum : uint32_t { ALG_SHA256_FIXED = 0, ALG_SHA256_ASN1 = 1, ALG_SHA384_ASN1 = 2 };
enum : uint8_t { KEY_LOADED = 0, KEY_BAD = 1 };

constexpr int kEntryWords = 30;                // (x, y) tight Montgomery digits and ten words of build space
constexpr int kTableWords = 8 * kEntryWords;   // the multiples 1..8: 960 bytes per key
constexpr int kRecWords = 17;                  // k_ecdsa_pack's record: r, s (8 words each), the early code

struct fe {
  uint32_t v[10];
};

constexpr uint32_t M28 = 0x0fffffffu;
constexpr uint32_t kNinvQ = 1u, kNinvN = 0xe00bc4fu;   // -1/q, -1/n mod 2^28

CESS_CONST uint32_t kQ[10] = {0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffu, 0x0u, 0x0u, 0x1000000u, 0x0u, 0xfffffffu, 0xfu};
CESS_CONST uint32_t kN[10] = {0xc632551u, 0xb9cac2fu, 0x79e84f3u, 0xfaada71u, 0xfffbce6u,
                              0xfffffffu, 0xffffffu,  0x0u,       0xfffffffu, 0xfu};
CESS_CONST uint32_t kQ32[10] = {0xfffffe0u, 0xfffffffu, 0xfffffffu, 0x1ffffu, 0x0u, 0x0u, 0x0u, 0x2u, 0xfffffe0u, 0x1ffu};
// R^2, R and b R mod q; R^2 and R mod n
CESS_CONST uint32_t kR2Q[10] = {0x50000u,   0x300000u,  0x0u,       0x0u,       0xffffffau,
                                0xfffffbfu, 0xffffeffu, 0xfffafffu, 0x2ffffu,   0x0u};
CESS_CONST uint32_t kR2N[10] = {0xfb36926u, 0x7fbc24cu, 0x36a7aeau, 0xa0a7b86u, 0x1d14956u,
                                0x9076ab5u, 0x1ec5961u, 0x84a3d0bu, 0x3b51c1eu, 0x8u};
CESS_CONST uint32_t kOneQ[10] = {0x1000000u, 0x0u,       0x0u,       0x0u,       0xfffff00u,
                                 0xfffffffu, 0xfffffffu, 0xfefffffu, 0xffffffu,  0x0u};
CESS_CONST uint32_t kOneN[10] = {0xf000000u, 0x39cdaau, 0xc46353du, 0xe8617b0u, 0x9055258u,
                                 0x431u,     0x0u,      0xff00000u, 0xffffffu,  0x0u};
CESS_CONST uint32_t kBm[10] = {0xfdc3006u, 0x29c4bddu, 0x89cdf62u, 0x542a90du, 0x5cc9cu,
                               0x2ed6acfu, 0xaabf721u, 0x3409721u, 0xde0b74eu, 0x1u};
// G in Montgomery digits, and its encoding (the context's base table is the key table of these bytes)
CESS_CONST uint32_t kGxm[10] = {0xc18905fu, 0x18a9143u, 0x9e730d4u, 0x5d57017u, 0xa95fc47u,
                                0x251075bu, 0x42b7762u, 0xc6616b1u, 0x6bdc7b4u, 0x7u};
CESS_CONST uint32_t kGym[10] = {0xa8571ffu, 0xce95560u, 0xdf25357u, 0xa7e55cdu, 0xab8e434u,
                                0xf3258b4u, 0x788dd21u, 0x854d768u, 0x8aafa5cu, 0x1u};
CESS_CONST uint8_t kGEnc[65] = {
    0x04, 0x6b, 0x17, 0xd1, 0xf2, 0xe1, 0x2c, 0x42, 0x47, 0xf8, 0xbc, 0xe6, 0xe5, 0x63, 0xa4, 0x40, 0xf2,
    0x77, 0x03, 0x7d, 0x81, 0x2d, 0xeb, 0x33, 0xa0, 0xf4, 0xa1, 0x39, 0x45, 0xd8, 0x98, 0xc2, 0x96, 0x4f,
    0xe3, 0x42, 0xe2, 0xfe, 0x1a, 0x7f, 0x9b, 0x8e, 0xe7, 0xeb, 0x4a, 0x7c, 0x0f, 0x9e, 0x16, 0x2b, 0xce,
    0x33, 0x57, 0x6b, 0x31, 0x5e, 0xce, 0xcb, 0xb6, 0x40, 0x68, 0x37, 0xbf, 0x51, 0xf5};
// n, q, q - n and the low half of n - 2 as little-endian 32-bit words
CESS_CONST uint32_t kNw[8] = {0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu,
                              0xffffffffu, 0xffffffffu, 0x00000000u, 0xffffffffu};
CESS_CONST uint32_t kQw[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0x00000000u,
                              0x00000000u, 0x00000000u, 0x00000001u, 0xffffffffu};
CESS_CONST uint32_t kQmNw[8] = {0x039cdaaeu, 0x0c46353du, 0x58e8617bu, 0x43190553u, 0u, 0u, 0u, 0u};
CESS_CONST uint32_t kNm2Low[4] = {0xfc63254fu, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu};
CESS_CONST uint32_t kQm2w[8] = {0xfffffffdu, 0xffffffffu, 0xffffffffu, 0x00000000u,
                                0x00000000u, 0x00000000u, 0x00000001u, 0xffffffffu};

// the bound on a column sum (the argument is in the file's head): 11 * 2^60 + 2^37
constexpr uint64_t kColBound = 11ull * (1ull << 60) + (1ull << 37);

// a column sum: 64 bits on the device; the host build shadows it in 128 bits
// and records the maximum (emu_ecdsa_col_max)
#if defined(CESS_HOSTEMU)
typedef unsigned __int128 col_t;
inline unsigned __int128 g_col_max = 0;
CESS_HD void col_seen(col_t c) {
  if (c > g_col_max) g_col_max = c;
}
#else
typedef uint64_t col_t;
CESS_HD void col_seen(col_t) {}
#endif

// pt_madd's special returns.  The host build counts how often each is taken
// (emu_ecdsa_madd_counts), so that a test row named after one can be held to
// it; the device build has no counter and no code for it.
#if defined(CESS_HOSTEMU)
enum { MADD_INF = 0, MADD_DBL = 1, MADD_CANCEL = 2 };
inline uint64_t g_madd_seen[3] = {0, 0, 0};
#define CESS_MADD_SEEN(which) (void)g_madd_seen[which]++
#else
#define CESS_MADD_SEEN(which) (void)0
#endif

CESS_HD fe fe_from(const uint32_t (&k)[10]) {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = k[i];
  return r;
}
CESS_HD fe fe_zero() {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = 0u;
  return r;
}
CESS_HD fe fe_select(bool c, const fe& a, const fe& b) {   // c ? a : b
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}

// ---------------------------------------------------------------------------
// Montgomery products modulo MOD (q or n): a b / 2^280, tight
// ---------------------------------------------------------------------------
template <const uint32_t (&MOD)[10], uint32_t NINV, class Col>
CESS_HD fe mont_cols(Col&& col) {
  uint32_t m[10];
  fe t;
  col_t acc = 0;
#pragma unroll
  for (int k = 0; k < 19; k++) {
    col(k, acc);
#pragma unroll
    for (int i = k < 10 ? 0 : k - 9; i < (k < 10 ? k : 10); i++)
      if (MOD[k - i] != 0u) acc += (uint64_t)m[i] * MOD[k - i];
    if (k < 10) {
      m[k] = (NINV == 1u ? (uint32_t)acc : (uint32_t)acc * NINV) & M28;
      acc += (uint64_t)m[k] * MOD[0];
    } else {
      t.v[k - 10] = (uint32_t)acc & M28;
    }
    col_seen(acc);
    acc >>= 28;
  }
  t.v[9] = (uint32_t)acc;
  return t;
}

template <const uint32_t (&MOD)[10], uint32_t NINV>
CESS_HD fe mont_mul(const fe& a, const fe& b) {
  return mont_cols<MOD, NINV>([&](int k, col_t& acc) {
#pragma unroll
    for (int i = 0; i < 10; i++)
      if (k - i >= 0 && k - i < 10) acc += (uint64_t)a.v[i] * b.v[k - i];
  });
}
// off-diagonal products once, against a doubled operand (digits below 2^31)
template <const uint32_t (&MOD)[10], uint32_t NINV>
CESS_HD fe mont_sqr(const fe& a) {
  uint32_t a2[10];
#pragma unroll
  for (int i = 0; i < 10; i++) a2[i] = a.v[i] << 1;
  return mont_cols<MOD, NINV>([&](int k, col_t& acc) {
#pragma unroll
    for (int i = 0; i < 10; i++) {
      const int j = k - i;
      if (j > i && j < 10) acc += (uint64_t)a.v[i] * a2[j];
    }
    if ((k & 1) == 0 && (k >> 1) < 10) acc += (uint64_t)a.v[k >> 1] * a.v[k >> 1];
  });
}

CESS_HD fe fe_mul(const fe& a, const fe& b) { return mont_mul<kQ, kNinvQ>(a, b); }
CESS_HD fe fe_sqr(const fe& a) { return mont_sqr<kQ, kNinvQ>(a); }
CESS_HD fe sc_mul(const fe& a, const fe& b) { return mont_mul<kN, kNinvN>(a, b); }
CESS_HD fe sc_sqr(const fe& a) { return mont_sqr<kN, kNinvN>(a); }

// acc^(2^nbits) x^e for the nbits-bit exponent e (words little-endian), most
// significant bit first
template <const uint32_t (&MOD)[10], uint32_t NINV, int W>
CESS_HD fe pow_bits(fe acc, const fe& x, const uint32_t (&e)[W]) {
#pragma unroll 1
  for (int w = W - 1; w >= 0; w--) {
    uint32_t bits = 0;
#pragma unroll
    for (int q = 0; q < W; q++) bits = q == w ? e[q] : bits;
#pragma unroll 1
    for (int b = 0; b < 32; b++) {
      acc = mont_sqr<MOD, NINV>(acc);
      if (bits >> 31) acc = mont_mul<MOD, NINV>(acc, x);
      bits <<= 1;
    }
  }
  return acc;
}

// ---------------------------------------------------------------------------
// the field mod q: sums and differences
// ---------------------------------------------------------------------------
CESS_HD fe fe_add(const fe& a, const fe& b) {   // lazy
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = a.v[i] + b.v[i];
  return r;
}

// v - floor(v / 2^256) q for carried digits (0..8 below 2^28, digit 9 below
// 2^10): below 2^256 + 2^230.  q = 2^256 - 2^224 + 2^192 + 2^96 - 1: the
// multiple's five terms go to digits 9, 8, 6, 3 and 0.
CESS_HD fe fe_weak(const fe& a) {
  const int32_t k = (int32_t)(a.v[9] >> 4);
  fe r;
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    int32_t t = (int32_t)a.v[i] + c;
    if (i == 0) t += k;
    if (i == 3) t -= k << 12;
    if (i == 6) t -= k << 24;
    if (i == 8) t += k;
    if (i == 9) t -= k << 4;
    r.v[i] = i < 9 ? (uint32_t)t & M28 : (uint32_t)t;
    c = t >> 28;
  }
  return r;
}

// a - b mod q for digits below 2^30 and b below 32 q: tight
CESS_HD fe fe_sub(const fe& a, const fe& b) {
  fe r;
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const int32_t t = (int32_t)a.v[i] - (int32_t)b.v[i] + (int32_t)kQ32[i] + c;
    r.v[i] = i < 9 ? (uint32_t)t & M28 : (uint32_t)t;
    c = t >> 28;
  }
  return fe_weak(r);
}
CESS_HD fe fe_neg(const fe& a) { return fe_sub(fe_zero(), a); }

// k a for a tight a and k <= 8: tight
CESS_HD fe fe_mulk(const fe& a, uint32_t k) {
  fe r;
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint32_t t = a.v[i] * k + c;
    r.v[i] = i < 9 ? t & M28 : t;
    c = t >> 28;
  }
  return fe_weak(r);
}

// a tight value is zero mod MOD iff it is 0 or MOD
template <const uint32_t (&MOD)[10]>
CESS_HD bool is_zero_mod(const fe& a) {
  uint32_t z = 0, q = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) z |= a.v[i], q |= a.v[i] ^ MOD[i];
  return z == 0 || q == 0;
}
CESS_HD bool fe_is_zero(const fe& a) { return is_zero_mod<kQ>(a); }
CESS_HD bool fe_eq(const fe& a, const fe& b) { return fe_is_zero(fe_sub(a, b)); }

// the canonical digits (value below MOD) of a tight value
template <const uint32_t (&MOD)[10]>
CESS_HD fe canon_mod(const fe& a) {
  fe d;
  int32_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const int32_t t = (int32_t)a.v[i] - (int32_t)MOD[i] + c;
    d.v[i] = i < 9 ? (uint32_t)t & M28 : (uint32_t)t;
    c = t >> 28;
  }
  return fe_select((int32_t)d.v[9] < 0, a, d);
}

// 8 little-endian words (a value below 2^256) <-> digits
CESS_HD fe digits_from_words(const uint32_t (&w)[8]) {
  fe r;
#pragma unroll
  for (int k = 0; k < 10; k++) {
    const int off = 28 * k, i = off >> 5, sh = off & 31;
    uint32_t lo = w[i] >> sh;
    if (sh > 4 && i + 1 < 8) lo |= w[i + 1] << (32 - sh);
    r.v[k] = lo & M28;
  }
  return r;
}
CESS_HD void words_from_digits(const fe& a, uint32_t (&w)[8]) {   // canonical digits
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int off = 32 * j, k = off / 28, sh = off - 28 * k;
    uint32_t x = a.v[k] >> sh;
    x |= a.v[k + 1] << (28 - sh);
    if (28 - sh + 28 < 32 && k + 2 < 10) x |= a.v[k + 2] << (56 - sh);
    w[j] = x;
  }
}

CESS_HD fe fe_to_mont(const fe& plain) { return fe_mul(plain, fe_from(kR2Q)); }
CESS_HD fe fe_from_mont(const fe& a) {
  fe one = fe_zero();
  one.v[0] = 1u;
  return canon_mod<kQ>(fe_mul(a, one));
}
CESS_HD fe sc_to_mont(const fe& plain) { return sc_mul(plain, fe_from(kR2N)); }
CESS_HD fe sc_from_mont(const fe& a) {
  fe one = fe_zero();
  one.v[0] = 1u;
  return canon_mod<kN>(sc_mul(a, one));
}

// z^(q - 2) (Montgomery form in and out): once per key
CESS_HD fe fe_invert(const fe& z) { return pow_bits<kQ, kNinvQ, 8>(fe_from(kOneQ), z, kQm2w); }

CESS_HD fe sc_sqn(fe x, int n) {
#pragma unroll 1
  for (int i = 0; i < n; i++) x = sc_sqr(x);
  return x;
}
// s^(n - 2) (Montgomery form in and out).  n - 2 = ffffffff 00000000 ffffffff
// ffffffff and 128 unstructured bits: 2^32 - 1 by doubling the run (5
// multiplies, 31 squarings), three more runs (96 squarings, 2 multiplies), the
// low half bit by bit (128 squarings, 73 multiplies).
CESS_HD fe sc_invert(const fe& s) {
  fe x = sc_mul(sc_sqr(s), s);               // 2^2 - 1
  x = sc_mul(sc_sqn(x, 2), x);               // 2^4 - 1
  x = sc_mul(sc_sqn(x, 4), x);               // 2^8 - 1
  x = sc_mul(sc_sqn(x, 8), x);               // 2^16 - 1
  x = sc_mul(sc_sqn(x, 16), x);              // 2^32 - 1
  fe acc = sc_mul(sc_sqn(x, 64), x);         // ffffffff 00000000 ffffffff
  acc = sc_mul(sc_sqn(acc, 32), x);
  return pow_bits<kN, kNinvN, 4>(acc, s, kNm2Low);
}

// ---------------------------------------------------------------------------
// integers as 8 little-endian words
// ---------------------------------------------------------------------------
CESS_HD bool words_lt(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)a[i] - b[i] - borrow;
    borrow = (uint32_t)(d >> 63);
  }
  return borrow != 0;
}
CESS_HD bool words_zero(const uint32_t (&a)[8]) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a[i];
  return o == 0;
}
// 32 big-endian bytes
CESS_HD void load_be(const uint8_t* b, uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint8_t* p = b + 28 - 4 * i;
    w[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
  }
}

// Rule 4: the leftmost 32 bytes of the digest as a big-endian integer, minus n
// once if it is at least n
CESS_HD void digest_scalar(const uint8_t* digest, uint32_t (&e)[8]) {
  load_be(digest, e);
  const bool ge = !words_lt(e, kNw);
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)e[i] - kNw[i] - borrow;
    borrow = (uint32_t)(d >> 63);
    e[i] = ge ? (uint32_t)d : e[i];
  }
}

// Signed radix-16 digits of s < 2^256: t = s + 0x88..8 (257 bits); digit i < 64
// is nibble i of t minus 8, in [-8, 7], and digit 64 is t's bit 256, 0 or 1.
// The ladder reads the top nibble of t[7] and shifts t left by 4 per round.
CESS_HD uint32_t sc_recode(const uint32_t (&s)[8], uint32_t (&t)[8]) {
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t x = (uint64_t)s[i] + 0x88888888u + carry;
    t[i] = (uint32_t)x;
    carry = (uint32_t)(x >> 32);
  }
  return carry;
}
CESS_HD int sc_top_digit(uint32_t (&t)[8]) {
  const int d = (int)(t[7] >> 28) - 8;
#pragma unroll
  for (int i = 7; i > 0; i--) t[i] = (t[i] << 4) | (t[i - 1] >> 28);
  t[0] <<= 4;
  return d;
}

// ---------------------------------------------------------------------------
// Rule 2: the signature's two integers
// ---------------------------------------------------------------------------
// ring's der::read_tag_and_get_value inside [at, end): tag and value range
CESS_HD bool der_tlv(const uint8_t* b, uint64_t end, uint64_t& at, uint32_t& tag, uint64_t& vb, uint64_t& ve) {
  if (end - at < 2) return false;
  tag = b[at];
  if ((tag & 0x1fu) == 0x1fu) return false;
  uint64_t len = b[at + 1];
  at += 2;
  if (len >= 0x80) {
    if (len == 0x81) {
      if (end - at < 1 || b[at] < 128) return false;
      len = b[at];
      at += 1;
    } else if (len == 0x82) {
      if (end - at < 2) return false;
      len = ((uint64_t)b[at] << 8) | b[at + 1];
      at += 2;
      if (len < 256) return false;
    } else {
      return false;
    }
  }
  if (end - at < len) return false;
  vb = at;
  ve = at + len;
  at = ve;
  return true;
}
// ring's der::positive_integer: the value's bytes without the leading zero
CESS_HD bool der_positive(const uint8_t* b, uint64_t end, uint64_t& at, uint64_t& vb, uint64_t& ve) {
  uint32_t tag;
  if (!der_tlv(b, end, at, tag, vb, ve) || tag != 0x02u || vb == ve) return false;
  if (b[vb] == 0) {
    if (ve - vb == 1 || (b[vb + 1] & 0x80) == 0) return false;   // zero; a leading zero not needed
    vb++;
    return true;
  }
  return (b[vb] & 0x80) == 0;                                      // negative
}
// the big-endian bytes [vb, ve), at most 32, as words
CESS_HD void words_from_be(const uint8_t* b, uint64_t vb, uint64_t ve, uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = 0;
  const uint32_t len = (uint32_t)(ve - vb);
#pragma unroll 1
  for (uint32_t q = 0; q < len; q++) {
    const uint32_t byte = b[ve - 1 - q], sh = 8 * (q & 3);
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] |= (uint32_t)i == (q >> 2) ? byte << sh : 0u;
  }
}
// Rules 2 and 3 of one signature: r and s, and EC_OK, EC_SIG_FORMAT or EC_SIG_RANGE
CESS_HD uint32_t parse_sig(uint32_t alg, const uint8_t* sig, uint64_t len, uint32_t (&r)[8], uint32_t (&s)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = s[i] = 0;
  bool wide = false;   // more than 32 significant bytes: at least 2^256
  if (alg == ALG_SHA256_FIXED) {
    if (len != 64) return EC_SIG_FORMAT;
    load_be(sig, r);
    load_be(sig + 32, s);
  } else {
    uint64_t at = 0, vb, ve, rb, re, sb, se;
    uint32_t tag;
    if (!der_tlv(sig, len, at, tag, vb, ve) || tag != 0x30u || at != len) return EC_SIG_FORMAT;
    at = vb;
    if (!der_positive(sig, ve, at, rb, re) || !der_positive(sig, ve, at, sb, se) || at != ve) return EC_SIG_FORMAT;
    wide = re - rb > 32 || se - sb > 32;
    if (!wide) {
      words_from_be(sig, rb, re, r);
      words_from_be(sig, sb, se, s);
    }
  }
  if (wide || words_zero(r) || words_zero(s) || !words_lt(r, kNw) || !words_lt(s, kNw)) return EC_SIG_RANGE;
  return EC_OK;
}

// ---------------------------------------------------------------------------
// the curve
// ---------------------------------------------------------------------------
struct jac {
  fe X, Y, Z;
};
CESS_HD jac pt_infinity() { return {fe_from(kOneQ), fe_from(kOneQ), fe_zero()}; }
CESS_HD bool pt_is_inf(const jac& p) { return fe_is_zero(p.Z); }

// 2 p (dbl-2001-b); infinity stays infinity (Z3 = 2 Y Z)
CESS_HD jac pt_dbl(const jac& p) {
  const fe delta = fe_sqr(p.Z), gamma = fe_sqr(p.Y);
  const fe beta = fe_mul(p.X, gamma);
  const fe alpha = fe_mul(fe_sub(p.X, delta), fe_add(p.X, delta));
  const fe alpha3 = fe_add(fe_add(alpha, alpha), alpha);            // lazy
  jac r;
  r.X = fe_sub(fe_sqr(alpha3), fe_mulk(beta, 8));
  r.Z = fe_sub(fe_sqr(fe_add(p.Y, p.Z)), fe_add(gamma, delta));
  r.Y = fe_sub(fe_mul(alpha3, fe_sub(fe_mulk(beta, 4), r.X)), fe_mulk(fe_sqr(gamma), 8));
  return r;
}

// p + (x2, y2) for an affine, finite second operand
CESS_HD jac pt_madd(const jac& p, const fe& x2, const fe& y2) {
  if (pt_is_inf(p)) {
    CESS_MADD_SEEN(MADD_INF);
    return {x2, y2, fe_from(kOneQ)};
  }
  const fe z1z1 = fe_sqr(p.Z);
  const fe u2 = fe_mul(x2, z1z1), s2 = fe_mul(y2, fe_mul(p.Z, z1z1));
  const fe h = fe_sub(u2, p.X), rr = fe_sub(s2, p.Y);
  if (fe_is_zero(h)) {
    if (fe_is_zero(rr)) {
      CESS_MADD_SEEN(MADD_DBL);
      return pt_dbl(p);
    }
    CESS_MADD_SEEN(MADD_CANCEL);
    return pt_infinity();
  }
  const fe hh = fe_sqr(h);
  const fe hhh = fe_mul(h, hh), v = fe_mul(p.X, hh);
  jac r;
  r.X = fe_sub(fe_sub(fe_sqr(rr), hhh), fe_add(v, v));
  r.Y = fe_sub(fe_mul(rr, fe_sub(v, r.X)), fe_mul(p.Y, hhh));
  r.Z = fe_mul(p.Z, h);
  return r;
}

CESS_HD void entry_load(const uint32_t* e, fe& x, fe& y) {
#if defined(CESS_HOSTEMU)
#pragma unroll
  for (int i = 0; i < 10; i++) x.v[i] = e[i], y.v[i] = e[10 + i];
#else
  const uint2* e2 = reinterpret_cast<const uint2*>(e);   // entries are 120 bytes: 8-byte aligned
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint2 a = e2[i], b = e2[5 + i];
    x.v[2 * i] = a.x, x.v[2 * i + 1] = a.y;
    y.v[2 * i] = b.x, y.v[2 * i + 1] = b.y;
  }
#endif
}
CESS_HD void fe_store(uint32_t* e, const fe& a) {
#pragma unroll
  for (int i = 0; i < 10; i++) e[i] = a.v[i];
}
CESS_HD fe fe_load(const uint32_t* e) {
  fe a;
#pragma unroll
  for (int i = 0; i < 10; i++) a.v[i] = e[i];
  return a;
}

// p + d Q from the table of Q's multiples 1..8, d in [-8, 8]; d = 0 adds nothing
CESS_HD jac pt_add_digit(const jac& p, const uint32_t* tab, int d) {
  if (d == 0) return p;
  const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
  fe x, y;
  entry_load(tab + kEntryWords * (ad - 1), x, y);
  if (d < 0) y = fe_neg(y);
  return pt_madd(p, x, y);
}

// Rule 1 and the table of one key: entries i Q, i = 1..8, affine Montgomery
// digits, normalised with one shared inversion.  `tab` (kTableWords words, this
// key's alone) also holds the Jacobian multiples between the two passes.  A key
// that does not load computes on G; its rows hold no usable values.
CESS_HD uint8_t key_table(const uint8_t* key, uint64_t len, uint32_t* tab) {
  bool ok = len == 65 && key[0] == 0x04;
  fe x = fe_from(kGxm), y = fe_from(kGym);
  if (ok) {
    uint32_t xw[8], yw[8];
    load_be(key + 1, xw);
    load_be(key + 33, yw);
    ok = words_lt(xw, kQw) && words_lt(yw, kQw);
    const fe xm = fe_to_mont(digits_from_words(xw)), ym = fe_to_mont(digits_from_words(yw));
    // y^2 = x^3 - 3 x + b
    const fe rhs = fe_sub(fe_add(fe_mul(fe_sqr(xm), xm), fe_from(kBm)), fe_add(fe_add(xm, xm), xm));
    ok = ok && fe_eq(fe_sqr(ym), rhs);
    x = fe_select(ok, xm, x);
    y = fe_select(ok, ym, y);
  }
  fe_store(tab, x);
  fe_store(tab + 10, y);
  fe_store(tab + 20, fe_zero());
  jac p = {x, y, fe_from(kOneQ)};
  // pass 1: multiples 2..8 as (X, Y, Z) in their rows; prefix products of Z in
  // registers (statically indexed: the loop counter selects by comparison)
  fe pre[7], run = fe_from(kOneQ);
#pragma unroll
  for (int k = 0; k < 7; k++) pre[k] = run;
#pragma unroll 1
  for (int i = 1; i < 8; i++) {
    p = pt_madd(p, x, y);   // (i = 1 takes the doubling branch)
    uint32_t* row = tab + kEntryWords * i;
    fe_store(row, p.X);
    fe_store(row + 10, p.Y);
    fe_store(row + 20, p.Z);
#pragma unroll
    for (int k = 0; k < 7; k++) pre[k] = fe_select(k == i - 1, run, pre[k]);   // product of the Z before row i
    run = fe_mul(run, p.Z);
  }
  fe inv = fe_invert(run);
  // pass 2, rows 8..2: 1 / Z_i = inv * pre_i, then inv *= Z_i
#pragma unroll 1
  for (int i = 7; i >= 1; i--) {
    uint32_t* row = tab + kEntryWords * i;
    const fe X = fe_load(row), Y = fe_load(row + 10), Z = fe_load(row + 20);
    fe pi = pre[0];
#pragma unroll
    for (int k = 1; k < 7; k++) pi = fe_select(k == i - 1, pre[k], pi);
    const fe zi = fe_mul(inv, pi);
    inv = fe_mul(inv, Z);
    const fe zi2 = fe_sqr(zi);
    fe_store(row, fe_mul(X, zi2));
    fe_store(row + 10, fe_mul(Y, fe_mul(zi2, zi)));
    fe_store(row + 20, fe_zero());
  }
  return ok ? KEY_LOADED : KEY_BAD;
}

// u1 G + u2 Q for u1, u2 below 2^256, from G's table and Q's: the ladder.  A
// zero digit reads no table row.
CESS_HD jac double_mul(const uint32_t* tab_q, const uint32_t* tab_g, const uint32_t (&u1)[8], const uint32_t (&u2)[8]) {
  uint32_t t1[8], t2[8];
  const uint32_t c1 = sc_recode(u1, t1), c2 = sc_recode(u2, t2);
  jac p = pt_infinity();
  p = pt_add_digit(p, tab_q, (int)c2);
  p = pt_add_digit(p, tab_g, (int)c1);
#pragma unroll 1
  for (int round = 0; round < 64; round++) {
#pragma unroll 1
    for (int j = 0; j < 4; j++) p = pt_dbl(p);
    const int dq = sc_top_digit(t2), dg = sc_top_digit(t1);
    p = pt_add_digit(p, tab_q, dq);
    p = pt_add_digit(p, tab_g, dg);
  }
  return p;
}

// Rules 5 and 6 on integers: e below n, r and s in [1, n - 1], the key's table
// and G's.
CESS_HD bool verify_scalars(const uint32_t* tab_q, const uint32_t* tab_g, const uint32_t (&e)[8],
                            const uint32_t (&r)[8], const uint32_t (&s)[8]) {
  uint32_t u1[8], u2[8];
  {
    const fe w = sc_invert(sc_to_mont(digits_from_words(s)));
    // (e / R) (w R) = e w, plain
    words_from_digits(canon_mod<kN>(sc_mul(digits_from_words(e), w)), u1);
    words_from_digits(canon_mod<kN>(sc_mul(digits_from_words(r), w)), u2);
  }
  const jac p = double_mul(tab_q, tab_g, u1, u2);
  if (pt_is_inf(p)) return false;
  // x(R) = r (mod n), as ring tests it: r Z^2 = X, then (r + n) Z^2 = X where r < q - n
  const fe z2 = fe_sqr(p.Z);
  if (fe_eq(fe_mul(fe_to_mont(digits_from_words(r)), z2), p.X)) return true;
  if (!words_lt(r, kQmNw)) return false;
  uint32_t rn[8], carry = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t x = (uint64_t)r[i] + kNw[i] + carry;
    rn[i] = (uint32_t)x;
    carry = (uint32_t)(x >> 32);
  }
  return fe_eq(fe_mul(fe_to_mont(digits_from_words(rn)), z2), p.X);
}

}  // namespace p256
