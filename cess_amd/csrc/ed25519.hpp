// Ed25519 verification under ring's rules (include/cess_ed25519.h,
// CESS_ED25519_POLICY_RING): GF(2^255 - 19), scalars mod L and the group, for
// k_ed25519_keys.hip, k_ed25519_verify.hip and the host build of the same code
// (tests/hostemu/ed25519_emu.cpp, -DCESS_HOSTEMU).  The rules are read from
// ring's ed25519/verification.rs and scalar.rs and from
// GFp_x25519_ge_frombytes_vartime; the code is this project's.
//
// Out of scope, on purpose: the chain's sp_io::crypto::ed25519_verify resolves
// to ed25519-zebra or ed25519-dalek 1.x, whose sources were not available to
// check.  From general knowledge (ZIP 215, the dalek 1.x source; UNVERIFIED
// here) zebra is cofactored and lenient on the encodings of R and A, and
// dalek 1.x checks only the top bits of S, so it does not reject every
// S >= L.  For signatures made
// by an honest signer all of them agree with the rules below; they differ on
// crafted inputs only.
//
// Field.  Ten unsaturated limbs of alternating 26 and 25 bits (radix 2^25.5:
// limb k has weight 2^ceil(25.5 k)), so 2^255 = 19 folds exactly at limb 10 and
// a product column needs no shift.  One limb product is one 32 x 32 + 64
// multiply-add (v_mad_u64_u32) into a lazy 64-bit column sum, as bls/field.hpp
// does for Fp381: a multiply is 100 multiply-adds (plus 9 32-bit multiplies by
// 19 and 5 doublings of operand limbs), a square 55 (plus 14 such scalings),
// each followed by one carry pass.  Bounds, all limbs unsigned:
//   tight   even limbs <= 2^26 + 2^12, odd limbs <= 2^25 + 2^16: what mul, sqr,
//           sub, neg and carry return
//   loose   twice that: what add returns for tight inputs
//   input   mul and sqr take limbs < 13 * 2^24 (even) and < 13 * 2^23 (odd), which
//           covers loose + tight; 19 * limb then fits 32 bits and a column
//           sum stays below 2^62.4 (the host build shadows every column sum in
//           128 bits and the test checks the maximum)
//   sub     a - b as a + 4p - b and a carry pass: b limbs up to the input bound
// Scalars are 8 x 32-bit words.  Points are extended coordinates (X, Y, Z, T);
// doubling works on (X, Y, Z) alone (dbl-2008-hwcd) and addition is mixed, with
// a precomputed affine entry (y + x, y - x, 2 d x y) (madd-2008-hwcd-3); both
// are complete on this curve (a = -1 is a square, d is not), so small-order
// keys and the identity need no special case.  The identity entry is (1, 1, 0).
#pragma once
#include <stdint.h>

#include "bls/field.hpp"   // CESS_HD, CESS_CONST

namespace ed25519 {

enum : uint32_t { ED_OK = 0, ED_SIG_LEN = 1, ED_SIG_RANGE = 2, ED_KEY = 3, ED_MISMATCH = 4 };
// per-key status of the table: loaded; not 32 bytes; does not decode
enum : uint8_t { KEY_LOADED = 0, KEY_BAD_LEN = 1, KEY_BAD_POINT = 2 };

constexpr int kEntryWords = 30;                  // (y + x, y - x, 2 d x y), 10 tight limbs each
constexpr int kTableWords = 8 * kEntryWords;     // the multiples 1..8: 960 bytes per key

struct fe {
  uint32_t v[10];
};

constexpr uint32_t M26 = (1u << 26) - 1, M25 = (1u << 25) - 1;
CESS_HD constexpr int limb_bits(int k) { return (k & 1) ? 25 : 26; }
CESS_HD constexpr uint32_t limb_mask(int k) { return (k & 1) ? M25 : M26; }

CESS_CONST uint32_t kD[10] = {0x35978a3u, 0xd37284u, 0x3156ebdu, 0x6a0a0eu, 0x1c029u,
                              0x179e898u, 0x3a03cbbu, 0x1ce7198u, 0x2e2b6ffu, 0x1480db3u};
CESS_CONST uint32_t kD2[10] = {0x2b2f159u, 0x1a6e509u, 0x22add7au, 0xd4141du, 0x38052u,
                               0xf3d130u, 0x3407977u, 0x19ce331u, 0x1c56dffu, 0x901b67u};
CESS_CONST uint32_t kSqrtM1[10] = {0x20ea0b0u, 0x186c9d2u, 0x8f189du, 0x35697fu, 0xbd0c60u,
                                   0x1fbd7a7u, 0x2804c9eu, 0x1e16569u, 0x4fc1du, 0xae0c92u};
// the encoding of -B (B: y = 4/5, x even; the sign bit set): its table, built
// like a key's, holds the multiples of -(-B) = B
CESS_CONST uint8_t kNegBaseEnc[32] = {0x58, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66,
                                   0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66,
                                   0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0x66, 0xe6};
// L = 2^252 + kC
CESS_CONST uint32_t kL[8] = {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0u, 0u, 0u, 0x10000000u};
CESS_CONST uint32_t kC[4] = {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu};

// a column sum: 64 bits on the device; the host build shadows it in 128 bits
// and records the maximum (emu_ed_col_max)
#if defined(CESS_HOSTEMU)
typedef unsigned __int128 col_t;
inline unsigned __int128 g_col_max = 0;
CESS_HD uint64_t col_out(col_t c) {
  if (c > g_col_max) g_col_max = c;
  return (uint64_t)c;
}
#else
typedef uint64_t col_t;
CESS_HD uint64_t col_out(col_t c) { return c; }
#endif

CESS_HD fe fe_from(const uint32_t (&k)[10]) {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = k[i];
  return r;
}
CESS_HD fe fe_small(uint32_t x) {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = i ? 0u : x;
  return r;
}

// one carry pass over ten column sums; the carry out of limb 9 comes back into
// limb 0 times 19 and once more into limb 1: tight
CESS_HD fe fe_from_cols(col_t (&h)[10]) {
  fe r;
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < 10; k++) {
    const uint64_t t = col_out(h[k] + c);
    r.v[k] = (uint32_t)t & limb_mask(k);
    c = t >> limb_bits(k);
  }
  const uint64_t t0 = r.v[0] + 19 * c;   // c < 2^40
  r.v[0] = (uint32_t)t0 & M26;
  r.v[1] += (uint32_t)(t0 >> 26);
  return r;
}

// 100 multiply-adds: column k takes f_i g_j for i + j = k and 19 f_i g_j for
// i + j = k + 10, doubled where i and j are both odd
CESS_HD fe fe_mul(const fe& f, const fe& g) {
  uint32_t g19[10], f2[10];
#pragma unroll
  for (int j = 0; j < 10; j++) g19[j] = 19u * g.v[j];
#pragma unroll
  for (int i = 0; i < 10; i++) f2[i] = 2u * f.v[i];
  col_t h[10];
#pragma unroll
  for (int k = 0; k < 10; k++) {
    col_t acc = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
      const int j = (k - i + 10) % 10;
      const uint32_t a = ((i & 1) && (j & 1)) ? f2[i] : f.v[i];
      const uint32_t b = i > k ? g19[j] : g.v[j];
      acc += (uint64_t)a * b;
    }
    h[k] = acc;
  }
  return fe_from_cols(h);
}

// 55 multiply-adds: the products i < j once, doubled
CESS_HD fe fe_sqr(const fe& f) {
  uint32_t f2[10], f19[10], f38[10];
#pragma unroll
  for (int i = 0; i < 10; i++) {
    f2[i] = 2u * f.v[i];
    f19[i] = 19u * f.v[i];
    f38[i] = 38u * f.v[i];   // used for odd i only
  }
  col_t h[10];
#pragma unroll
  for (int k = 0; k < 10; k++) {
    col_t acc = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
      const int j = (k - i + 10) % 10;
      if (i > j) continue;
      const bool wrap = i + j >= 10, odd2 = (i & 1) && (j & 1);
      const uint32_t a = i == j ? f.v[i] : f2[i];
      const uint32_t b = wrap ? (odd2 ? f38[j] : f19[j]) : (odd2 ? f2[j] : f.v[j]);
      acc += (uint64_t)a * b;
    }
    h[k] = acc;
  }
  return fe_from_cols(h);
}

CESS_HD fe fe_sqn(fe x, int n) {
#pragma unroll 1
  for (int i = 0; i < n; i++) x = fe_sqr(x);
  return x;
}

CESS_HD fe fe_add(const fe& a, const fe& b) {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = a.v[i] + b.v[i];
  return r;
}

// 32-bit carry pass (limbs < 2^32 - 2^7): tight
CESS_HD fe fe_carry(const fe& a) {
  fe r;
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < 10; k++) {
    const uint32_t t = a.v[k] + c;
    r.v[k] = t & limb_mask(k);
    c = t >> limb_bits(k);
  }
  r.v[0] += 19u * c;
  return r;
}

// a - b: a + 4p - b, carried
CESS_HD fe fe_sub(const fe& a, const fe& b) {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint32_t p4 = i == 0 ? (1u << 28) - 76u : (i & 1) ? (1u << 27) - 4u : (1u << 28) - 4u;
    r.v[i] = a.v[i] + p4 - b.v[i];
  }
  return fe_carry(r);
}
CESS_HD fe fe_neg(const fe& a) { return fe_sub(fe_small(0), a); }

// 2p - a for a tight a, without a carry pass: loose
CESS_HD fe fe_neg_tight(const fe& a) {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint32_t p2 = i == 0 ? (1u << 27) - 38u : (i & 1) ? (1u << 26) - 2u : (1u << 27) - 2u;
    r.v[i] = p2 - a.v[i];
  }
  return r;
}

CESS_HD fe fe_select(bool c, const fe& a, const fe& b) {   // c ? a : b
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}

// 8 little-endian words -> limbs (bit 255 is dropped; values up to 2^255 - 1
// are taken as they are: no canonical check)
CESS_HD fe fe_from_words(const uint32_t (&w)[8]) {
  fe r;
  r.v[0] = w[0] & M26;
  r.v[1] = ((w[0] >> 26) | (w[1] << 6)) & M25;
  r.v[2] = ((w[1] >> 19) | (w[2] << 13)) & M26;
  r.v[3] = ((w[2] >> 13) | (w[3] << 19)) & M25;
  r.v[4] = (w[3] >> 6) & M26;
  r.v[5] = w[4] & M25;
  r.v[6] = ((w[4] >> 25) | (w[5] << 7)) & M26;
  r.v[7] = ((w[5] >> 19) | (w[6] << 13)) & M25;
  r.v[8] = ((w[6] >> 12) | (w[7] << 20)) & M26;
  r.v[9] = (w[7] >> 6) & M25;
  return r;
}

// the canonical value (< p) of a limb vector within the input bound, as 8 words
CESS_HD void fe_to_words(const fe& a, uint32_t (&w)[8]) {
  // two carry passes: every limb strictly within its bits, value < 2^255
  fe t = fe_carry(fe_carry(a));
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < 10; k++) {
    const uint32_t s = t.v[k] + c;
    t.v[k] = s & limb_mask(k);
    c = s >> limb_bits(k);
  }
  t.v[0] += 19u * c;   // c = 1 only where the rest is tiny: no further carry
  // q = 1 iff t >= p, i.e. iff t + 19 reaches 2^255
  uint32_t q = (t.v[0] + 19u) >> 26;
#pragma unroll
  for (int k = 1; k < 10; k++) q = (t.v[k] + q) >> limb_bits(k);
  c = 19u * q;
#pragma unroll
  for (int k = 0; k < 10; k++) {
    const uint32_t s = t.v[k] + c;
    t.v[k] = s & limb_mask(k);   // the carry out of limb 9 is the subtracted 2^255
    c = s >> limb_bits(k);
  }
  w[0] = t.v[0] | (t.v[1] << 26);
  w[1] = (t.v[1] >> 6) | (t.v[2] << 19);
  w[2] = (t.v[2] >> 13) | (t.v[3] << 13);
  w[3] = (t.v[3] >> 19) | (t.v[4] << 6);
  w[4] = t.v[5] | (t.v[6] << 25);
  w[5] = (t.v[6] >> 7) | (t.v[7] << 19);
  w[6] = (t.v[7] >> 13) | (t.v[8] << 12);
  w[7] = (t.v[8] >> 20) | (t.v[9] << 6);
}

CESS_HD bool fe_is_zero(const fe& a) {
  uint32_t w[8], o = 0;
  fe_to_words(a, w);
#pragma unroll
  for (int i = 0; i < 8; i++) o |= w[i];
  return o == 0;
}
CESS_HD uint32_t fe_is_negative(const fe& a) {
  uint32_t w[8];
  fe_to_words(a, w);
  return w[0] & 1u;
}

// z^(p - 2): 254 squarings, 11 multiplies
CESS_HD fe fe_invert(const fe& z) {
  fe t0 = fe_sqr(z);
  fe t1 = fe_sqn(t0, 2);
  t1 = fe_mul(z, t1);            // z^9
  t0 = fe_mul(t0, t1);           // z^11
  fe t2 = fe_sqr(t0);
  t1 = fe_mul(t1, t2);           // z^(2^5 - 1)
  t2 = fe_sqn(t1, 5);
  t1 = fe_mul(t2, t1);           // 2^10 - 1
  t2 = fe_sqn(t1, 10);
  t2 = fe_mul(t2, t1);           // 2^20 - 1
  fe t3 = fe_sqn(t2, 20);
  t2 = fe_mul(t3, t2);           // 2^40 - 1
  t2 = fe_sqn(t2, 10);
  t1 = fe_mul(t2, t1);           // 2^50 - 1
  t2 = fe_sqn(t1, 50);
  t2 = fe_mul(t2, t1);           // 2^100 - 1
  t3 = fe_sqn(t2, 100);
  t2 = fe_mul(t3, t2);           // 2^200 - 1
  t2 = fe_sqn(t2, 50);
  t1 = fe_mul(t2, t1);           // 2^250 - 1
  t1 = fe_sqn(t1, 5);
  return fe_mul(t1, t0);         // 2^255 - 21
}

// z^((p - 5) / 8) = z^(2^252 - 3): 251 squarings, 12 multiplies
CESS_HD fe fe_pow22523(const fe& z) {
  fe t0 = fe_sqr(z);
  fe t1 = fe_sqn(t0, 2);
  t1 = fe_mul(z, t1);            // z^9
  t0 = fe_mul(t0, t1);           // z^11
  t0 = fe_sqr(t0);
  t0 = fe_mul(t1, t0);           // 2^5 - 1
  t1 = fe_sqn(t0, 5);
  t0 = fe_mul(t1, t0);           // 2^10 - 1
  t1 = fe_sqn(t0, 10);
  t1 = fe_mul(t1, t0);           // 2^20 - 1
  fe t2 = fe_sqn(t1, 20);
  t1 = fe_mul(t2, t1);           // 2^40 - 1
  t1 = fe_sqn(t1, 10);
  t0 = fe_mul(t1, t0);           // 2^50 - 1
  t1 = fe_sqn(t0, 50);
  t1 = fe_mul(t1, t0);           // 2^100 - 1
  t2 = fe_sqn(t1, 100);
  t1 = fe_mul(t2, t1);           // 2^200 - 1
  t1 = fe_sqn(t1, 50);
  t0 = fe_mul(t1, t0);           // 2^250 - 1
  t0 = fe_sqn(t0, 2);
  return fe_mul(t0, z);          // 2^252 - 3
}

// ---------------------------------------------------------------------------
// scalars: 8 little-endian 32-bit words
// ---------------------------------------------------------------------------
CESS_HD bool sc_lt_L(const uint32_t (&s)[8]) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)s[i] - kL[i] - borrow;
    borrow = (uint32_t)(d >> 63);
  }
  return borrow != 0;
}

// out[0 .. NA + NB) = a * b (row by row: no intermediate exceeds 64 bits)
template <int NA, int NB>
CESS_HD void sc_mul(const uint32_t (&a)[NA], const uint32_t (&b)[NB], uint32_t (&out)[NA + NB]) {
#pragma unroll
  for (int i = 0; i < NA + NB; i++) out[i] = 0;
#pragma unroll
  for (int i = 0; i < NA; i++) {
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const uint64_t t = (uint64_t)a[i] * b[j] + out[i + j] + carry;
      out[i + j] = (uint32_t)t;
      carry = (uint32_t)(t >> 32);
    }
    out[i + NB] = carry;
  }
}

// x mod L for a 512-bit x.  2^252 = -c (mod L) with c = kC of 125 bits:
//   x = x_lo + 2^252 x_hi            x_hi < 2^260
//   c x_hi = y_lo + 2^252 y_hi       y_hi < 2^133
//   c y_hi = z_lo + 2^252 z_hi       z_hi < 2^6
// so x = x_lo - y_lo + z_lo - c z_hi (mod L), every term below 2^252: add 2 L
// and subtract L while the value is at least L (at most three times).
CESS_HD void sc_reduce512(const uint32_t (&x)[16], uint32_t (&out)[8]) {
  uint32_t xhi[9], y[13], yhi[5], z[9], w[5];
#pragma unroll
  for (int i = 0; i < 8; i++) xhi[i] = (x[7 + i] >> 28) | (x[8 + i] << 4);
  xhi[8] = x[15] >> 28;
  sc_mul<9, 4>(xhi, kC, y);
#pragma unroll
  for (int i = 0; i < 4; i++) yhi[i] = (y[7 + i] >> 28) | (y[8 + i] << 4);
  yhi[4] = (y[11] >> 28) | (y[12] << 4);
  sc_mul<5, 4>(yhi, kC, z);
  const uint32_t zhi1[1] = {(z[7] >> 28) | (z[8] << 4)};
  sc_mul<1, 4>(zhi1, kC, w);
  // v = x_lo + z_lo + 2 L - y_lo - c z_hi, in 9 words with a signed running carry
  int64_t c = 0;
  uint32_t v[9];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    int64_t t = c;
    if (i < 8) {
      const uint32_t m = i == 7 ? 0x0fffffffu : 0xffffffffu;
      t += (int64_t)(x[i] & m) + (int64_t)(z[i] & m) - (int64_t)(y[i] & m);
      t += 2 * (int64_t)kL[i];
    }
    if (i < 5) t -= (int64_t)w[i];
    v[i] = (uint32_t)t;
    c = t >> 32;
  }
  // 0 <= v < 4 L
#pragma unroll
  for (int r = 0; r < 3; r++) {
    uint32_t d[9], borrow = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const uint64_t t = (uint64_t)v[i] - (i < 8 ? kL[i] : 0u) - borrow;
      d[i] = (uint32_t)t;
      borrow = (uint32_t)(t >> 63);
    }
#pragma unroll
    for (int i = 0; i < 9; i++) v[i] = borrow ? v[i] : d[i];
  }
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = v[i];
}

// Signed radix-16 digits of s < 2^255: r = s + 0x88..8; digit i is nibble i of r
// minus 8, in [-8, 7].  The verify loop reads the top nibble of r[7] and shifts
// r left by 4 per round, so no word is indexed by a loop counter.
CESS_HD void sc_recode(const uint32_t (&s)[8], uint32_t (&r)[8]) {
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)s[i] + 0x88888888u + carry;
    r[i] = (uint32_t)t;
    carry = (uint32_t)(t >> 32);
  }
}
CESS_HD int sc_top_digit(uint32_t (&r)[8]) {
  const int d = (int)(r[7] >> 28) - 8;
#pragma unroll
  for (int i = 7; i > 0; i--) r[i] = (r[i] << 4) | (r[i - 1] >> 28);
  r[0] <<= 4;
  return d;
}

// ---------------------------------------------------------------------------
// group
// ---------------------------------------------------------------------------
struct ge_p3 {
  fe X, Y, Z, T;
};
struct ge_pre {
  fe ypx, ymx, xy2d;
};

// 2 (X : Y : Z) as the four factors (E, H, G, F): X3 = E F, Y3 = G H,
// Z3 = F G, T3 = E H.  4 squarings.
CESS_HD void ge_dbl(const ge_p3& p, fe& E, fe& H, fe& G, fe& F) {
  const fe xx = fe_sqr(p.X), yy = fe_sqr(p.Y), zz = fe_sqr(p.Z);
  const fe a = fe_sqr(fe_add(p.X, p.Y));
  H = fe_add(yy, xx);                 // loose
  G = fe_sub(yy, xx);
  E = fe_sub(a, H);
  F = fe_sub(fe_add(zz, zz), G);
}
// p + q for an affine entry q, as the same four factors.  3 multiplies.
CESS_HD void ge_madd(const ge_p3& p, const ge_pre& q, fe& E, fe& H, fe& G, fe& F) {
  const fe a = fe_mul(fe_add(p.Y, p.X), q.ypx);
  const fe b = fe_mul(fe_sub(p.Y, p.X), q.ymx);
  const fe c = fe_mul(q.xy2d, p.T);
  const fe d = fe_add(p.Z, p.Z);      // loose
  E = fe_sub(a, b);
  H = fe_add(a, b);                   // loose
  G = fe_add(d, c);                   // loose + tight: within the input bound
  F = fe_sub(d, c);
}
CESS_HD void ge_finish(ge_p3& p, const fe& E, const fe& H, const fe& G, const fe& F, bool with_t) {
  p.X = fe_mul(E, F);
  p.Y = fe_mul(G, H);
  p.Z = fe_mul(F, G);
  if (with_t) p.T = fe_mul(E, H);
}

CESS_HD ge_pre ge_pre_identity() { return {fe_small(1), fe_small(1), fe_small(0)}; }

CESS_HD ge_pre ge_pre_load(const uint32_t* e) {
  ge_pre q;
#if defined(CESS_HOSTEMU)
#pragma unroll
  for (int i = 0; i < 10; i++) q.ypx.v[i] = e[i], q.ymx.v[i] = e[10 + i], q.xy2d.v[i] = e[20 + i];
#else
  const uint2* e2 = reinterpret_cast<const uint2*>(e);   // entries are 120 bytes: 8-byte aligned
  uint32_t w[kEntryWords];
#pragma unroll
  for (int i = 0; i < kEntryWords / 2; i++) {
    const uint2 t = e2[i];
    w[2 * i] = t.x;
    w[2 * i + 1] = t.y;
  }
#pragma unroll
  for (int i = 0; i < 10; i++) q.ypx.v[i] = w[i], q.ymx.v[i] = w[10 + i], q.xy2d.v[i] = w[20 + i];
#endif
  return q;
}
CESS_HD void ge_pre_store(uint32_t* e, const fe& a, const fe& b, const fe& c) {
#pragma unroll
  for (int i = 0; i < 10; i++) e[i] = a.v[i], e[10 + i] = b.v[i], e[20 + i] = c.v[i];
}

// the entry d * Q of a table of Q's multiples 1..8 for a digit d in [-8, 8]:
// a zero digit selects the identity entry (the row of multiple 1 is read and
// replaced), a negative one swaps y + x with y - x and negates 2 d x y
CESS_HD ge_pre ge_pre_digit(const uint32_t* tab, int d) {
  const bool neg = d < 0;
  const uint32_t ad = (uint32_t)(neg ? -d : d);
  ge_pre q = ge_pre_load(tab + kEntryWords * (ad ? ad - 1 : 0));
  const ge_pre one = ge_pre_identity();
  q.ypx = fe_select(ad != 0, q.ypx, one.ypx);
  q.ymx = fe_select(ad != 0, q.ymx, one.ymx);
  q.xy2d = fe_select(ad != 0, q.xy2d, one.xy2d);
  ge_pre r;
  r.ypx = fe_select(neg, q.ymx, q.ypx);
  r.ymx = fe_select(neg, q.ypx, q.ymx);
  r.xy2d = fe_select(neg, fe_neg_tight(q.xy2d), q.xy2d);
  return r;
}

// Rule 4: A from 32 bytes given as 8 words.  y is the low 255 bits as they are
// (an encoding of y + p is accepted); x by RFC 8032 §5.1.3; if x's parity
// differs from bit 255, x is negated (x = 0 stays 0 and is accepted).  False
// if no root exists.
CESS_HD bool ge_decode(const uint32_t (&w)[8], fe& x, fe& y) {
  y = fe_from_words(w);
  const fe one = fe_small(1);
  const fe yy = fe_sqr(y);
  const fe u = fe_sub(yy, one);
  const fe v = fe_add(fe_mul(yy, fe_from(kD)), one);   // loose
  const fe v3 = fe_mul(fe_sqr(v), v);
  const fe uv7 = fe_mul(fe_mul(fe_sqr(v3), v), u);
  x = fe_mul(fe_mul(fe_pow22523(uv7), v3), u);
  const fe vxx = fe_mul(fe_sqr(x), v);
  // v x^2 = u: x is the root; = -u: x sqrt(-1) is; neither: there is none
  const bool direct = fe_is_zero(fe_sub(vxx, u)), flipped = fe_is_zero(fe_add(vxx, u));
  x = fe_select(direct, x, fe_mul(x, fe_from(kSqrtM1)));
  x = fe_select(fe_is_negative(x) != (w[7] >> 31), fe_neg(x), x);
  return direct || flipped;
}

CESS_HD void load_words(const uint8_t* b, uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++)
    w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
           ((uint32_t)b[4 * i + 3] << 24);
}

// The table of one key: entries i * (-A), i = 1..8, affine, normalised with one
// shared inversion.  `tab` (kTableWords words, this key's alone) also holds the
// projective multiples between the two passes.  Returns the key's status; the
// rows of a key that did not load hold no usable values.
CESS_HD uint8_t key_table(const uint8_t* key, uint64_t len, uint32_t* tab) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = i ? 0u : 1u;   // a key of another length computes on the identity
  if (len == 32) load_words(key, w);
  fe x, y;
  const bool ok = ge_decode(w, x, y);
  x = fe_neg(x);                                   // -A
  const fe d2 = fe_from(kD2);
  ge_pre e1;
  e1.ypx = fe_carry(fe_add(y, x));
  e1.ymx = fe_sub(y, x);
  const fe xy = fe_mul(x, y);
  e1.xy2d = fe_mul(xy, d2);
  ge_pre_store(tab, e1.ypx, e1.ymx, e1.xy2d);
  ge_p3 p = {x, y, fe_small(1), xy};
  // pass 1: multiples 2..8 as (X, Y, Z) in their rows; prefix products of Z in
  // registers (statically indexed: the loop counter selects by comparison)
  fe pre[7], run = fe_small(1);
#pragma unroll
  for (int k = 0; k < 7; k++) pre[k] = run;
#pragma unroll 1
  for (int i = 1; i < 8; i++) {
    fe E, H, G, F;
    ge_madd(p, e1, E, H, G, F);
    ge_finish(p, E, H, G, F, true);
    ge_pre_store(tab + kEntryWords * i, p.X, p.Y, p.Z);
#pragma unroll
    for (int k = 0; k < 7; k++) pre[k] = fe_select(k == i - 1, run, pre[k]);   // product of the Z before row i
    run = fe_mul(run, p.Z);
  }
  fe inv = fe_invert(run);
  // pass 2, rows 8..2: 1 / Z_i = inv * pre_i, then inv *= Z_i
#pragma unroll 1
  for (int i = 7; i >= 1; i--) {
    uint32_t* row = tab + kEntryWords * i;
    fe X, Y, Z, pi = pre[0];
#pragma unroll
    for (int k = 0; k < 10; k++) X.v[k] = row[k], Y.v[k] = row[10 + k], Z.v[k] = row[20 + k];
#pragma unroll
    for (int k = 1; k < 7; k++) pi = fe_select(k == i - 1, pre[k], pi);
    const fe zi = fe_mul(inv, pi);
    inv = fe_mul(inv, Z);
    const fe ax = fe_mul(X, zi), ay = fe_mul(Y, zi);
    ge_pre_store(row, fe_carry(fe_add(ay, ax)), fe_sub(ay, ax), fe_mul(fe_mul(ax, ay), d2));
  }
  return len != 32 ? KEY_BAD_LEN : ok ? KEY_LOADED : KEY_BAD_POINT;
}

// Codes 1..3 of a record, in the order of include/cess_ed25519.h: KEY for a
// missing or short key, SIG_LEN, SIG_RANGE, KEY for a key that did not decode.
// key_status: the table's, or KEY_BAD_LEN for an index outside it.
CESS_HD uint32_t early_code(uint8_t key_status, uint64_t sig_len, const uint32_t (&S)[8]) {
  if (key_status == KEY_BAD_LEN) return ED_KEY;
  if (sig_len != 64) return ED_SIG_LEN;
  if (!sc_lt_L(S)) return ED_SIG_RANGE;
  if (key_status != KEY_LOADED) return ED_KEY;
  return ED_OK;
}

// R' = [S]B + [h](-A) for reduced S and h, compared with R: 64 rounds of four
// doublings and two mixed additions.  Every lane runs every round: a lane whose
// record already has a code is given zero scalars and tab_b for both tables.
CESS_HD bool verify_equation(const uint32_t* tab_a, const uint32_t* tab_b, const uint32_t (&S)[8],
                             const uint32_t (&h)[8], const uint32_t (&R)[8]) {
  uint32_t rs[8], rh[8];
  sc_recode(S, rs);
  sc_recode(h, rh);
  ge_p3 p = {fe_small(0), fe_small(1), fe_small(1), fe_small(0)};
#pragma unroll 1
  for (int round = 0; round < 64; round++) {
    fe E, H, G, F;
    if (round) {   // (the first round would double the identity)
#pragma unroll 1
      for (int j = 0; j < 4; j++) {
        ge_dbl(p, E, H, G, F);
        ge_finish(p, E, H, G, F, j == 3);
      }
    }
    const int dh = sc_top_digit(rh), ds = sc_top_digit(rs);
#pragma unroll 1
    for (int t = 0; t < 2; t++) {
      const ge_pre q = ge_pre_digit(t ? tab_b : tab_a, t ? ds : dh);
      ge_madd(p, q, E, H, G, F);
      ge_finish(p, E, H, G, F, t == 0);
    }
  }
  const fe zi = fe_invert(p.Z);
  const fe x = fe_mul(p.X, zi), y = fe_mul(p.Y, zi);
  uint32_t w[8], diff = 0;
  fe_to_words(y, w);
  w[7] |= fe_is_negative(x) << 31;
#pragma unroll
  for (int i = 0; i < 8; i++) diff |= w[i] ^ R[i];
  return diff == 0;
}

}  // namespace ed25519
