// EMSA-PSS-VERIFY of one record, as ring 0.16.9 does it for
// RSA_PSS_2048_8192_SHA256 / _SHA384 / _SHA512 (reference
// utils/ring/src/rsa/padding.rs:307-487: salt length = digest length, MGF1 over
// the same digest), on the message value m = s^e mod n that the exponentiation
// kernels' store mode leaves behind (k_rsa.hpp, k_rsa_big.hip).  Shared by
// k_rsa_pss.hip and the host build of the same code
// (tests/hostemu/rsa_pss_emu.cpp).
//
// m is read as little-endian 32-bit words (word 0 = the least significant);
// byte i of m, counted from the least significant end, is EM[em_len - 1 - i]:
//   i = 0                 the trailer 0xbc
//   i = 1 .. h            H' (H'[0] at i = h)
//   i = h + 1 .. em_len-1 maskedDB (DB[0] at i = em_len - 1)
//   i = em_len .. k - 1   zero (one byte, where 8 divides mod_bits - 1)
// A big-endian 32-bit word of EM -- what SHA-2 consumes -- whose last byte is
// byte `pos` of m is bits [8 pos, 8 pos + 32) of m: a funnel shift of two
// neighbouring words of m, with no byte swap.
//
// Two alignments.  Everything that is placed from the END of EM has a fixed
// byte phase in the words of m: H' and the salt (the last h bytes of DB, which
// ends where H' starts) both start one byte above a word boundary, so their
// words are (w[q + 1] : w[q]) >> 8 with compile-time q.  The MGF1 mask is
// counted from the START of DB, em_len - 1 - h bytes above that, so the phase of
// mask words against words of m is em_len & 3, a per-key value: the padding
// check walks DB from its start in mask order and fetches m through a funnel
// shift by that amount.  The salt is then taken in m's phase, and its mask
// -- the last h bytes of the mask, which lie in the last two MGF1 blocks --
// is brought there by a word barrel shift and a byte funnel over those two
// blocks' digests (no byte loop, no run-time register index).
//
// Compressions per record: ceil((em_len - h - 1) / h) for MGF1 (its input,
// h + 4 bytes, is one block for every digest) and the final hash over
// 8 + 2 h bytes: two blocks for SHA-256 and SHA-512, one for SHA-384.
//
// The MGF1 trip count depends on the key, so lanes of one wave leave the loop
// at different times; nothing in it is wave-collective.
#pragma once
#include <stdint.h>

#include "rsa.hpp"
#include "rsa_digest.hpp"
#include "rsa_digest512.hpp"

namespace rsa_pss {

// the three hashes as the check needs them: h bytes = kHW big-endian 32-bit
// words of digest, blocks of kBlkW words, a length field that ends the block
struct P256 {
  using word = uint32_t;
  static constexpr int kHW = 8, kBlkW = 16;
  static CESS_HD void init(word (&st)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = bls::SHA_IV[j];
  }
  static CESS_HD void compress(word (&st)[8], const uint32_t (&blk)[16]) { bls::sha256_compress(st, blk); }
  static CESS_HD uint32_t out(const word (&st)[8], int j) { return st[j]; }
};
template <int DIGEST>
struct P512 {
  using word = uint64_t;
  static constexpr int kHW = DIGEST == rsa_digest512::kSha384 ? 12 : 16, kBlkW = 32;
  static CESS_HD void init(word (&st)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = rsa_digest512::Sha512::iv(DIGEST, j);
  }
  static CESS_HD void compress(word (&st)[8], const uint32_t (&blk)[32]) { rsa_digest512::sha512_compress(st, blk); }
  static CESS_HD uint32_t out(const word (&st)[8], int j) {
    return (j & 1) ? (uint32_t)st[j >> 1] : (uint32_t)(st[j >> 1] >> 32);
  }
};
using P384 = P512<rsa_digest512::kSha384>;
using P512f = P512<rsa_digest512::kSha512>;

// bits [8 s, 8 s + 32) of hi : lo, s = 0..3 (a lane-variable funnel shift)
CESS_HD uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t s) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * s));
}

// mw(j): word j of m (0 for words past the k bytes); mh: H(msg) as big-endian
// words.  RSA_OK or RSA_MISMATCH (ring's Unspecified).
template <class P, class F>
CESS_HD uint8_t check(F mw, uint32_t mod_bits, uint32_t k, const uint32_t (&mh)[P::kHW]) {
  constexpr int HW = P::kHW, BW = P::kBlkW;
  constexpr uint32_t h = 4 * HW;
  if (mod_bits < 2) return RSA_MISMATCH;
  const uint32_t em_bits = mod_bits - 1, em_len = (em_bits + 7) / 8;
  const uint32_t top_mask = 0xffu >> (8 * em_len - em_bits);
  if (em_len < 2 * h + 2) return RSA_MISMATCH;   // PSSMetrics::new fails
  const uint32_t db_len = em_len - h - 1, ps_len = db_len - h - 1;
  bool bad = false;
  // the byte above EM, where there is one (top_byte_mask == 0xff)
  if (em_len < k) bad = ((mw((k - 1) >> 2) >> (8 * ((k - 1) & 3))) & 0xff) != 0;
  // trailer, H'
  uint32_t hp[HW];
  {
    uint32_t hi = mw(HW);
#pragma unroll
    for (int t = 0; t < HW; t++) {
      const uint32_t lo = mw(HW - 1 - t);
      hp[t] = (hi << 24) | (lo >> 8);
      hi = lo;
    }
    bad = bad || (hi & 0xff) != 0xbc;
  }
  // MGF1 block b = H(H' || be32(b)); DB from its start, in mask order, up to
  // the separator: DB word u = bytes 4 u .. 4 u + 3 of DB ends at byte
  // em_len - 4 - 4 u of m
  const uint32_t nblk = (db_len + h - 1) / h;
  const uint32_t q0 = (em_len - 4) >> 2, sh = (em_len - 4) & 3;
  uint32_t hi = mw(q0 + 1);
  uint32_t prev[HW], cur[HW];
#pragma unroll
  for (int t = 0; t < HW; t++) cur[t] = 0;
  uint32_t u = 0;
#pragma unroll 1
  for (uint32_t b = 0; b < nblk; b++) {
    uint32_t blk[BW];
#pragma unroll
    for (int t = 0; t < HW; t++) blk[t] = hp[t], prev[t] = cur[t];
    blk[HW] = b;
    blk[HW + 1] = 0x80000000u;
#pragma unroll
    for (int t = HW + 2; t < BW - 1; t++) blk[t] = 0;
    blk[BW - 1] = 8 * (h + 4);
    typename P::word st[8];
    P::init(st);
    P::compress(st, blk);
#pragma unroll
    for (int t = 0; t < HW; t++) {
      cur[t] = P::out(st, t);
      if (4 * u <= ps_len) {   // the word holds a padding byte or the separator
        const uint32_t lo = mw(q0 - u);
        uint32_t d = funnel(hi, lo, sh);
        hi = lo;
        if (u == 0) bad = bad || ((d >> 24) & ~top_mask) != 0;
        d ^= cur[t];
        if (u == 0) d &= (top_mask << 24) | 0x00ffffffu;
        const uint32_t rel = ps_len - 4 * u;   // the separator's byte in this word, if < 4
        const uint32_t zmask = rel >= 3 ? 0xffffffffu : ~(0xffffffffu >> (8 * (rel + 1)));
        const uint32_t want = rel > 3 ? 0u : 1u << (8 * (3 - rel));
        bad = bad || (d & zmask) != want;
      }
      u++;
    }
  }
  // the salt's mask: bytes r .. r + h of prev || cur (blocks nblk - 2 and
  // nblk - 1; nblk >= 2 because db_len > h), r = 1 .. h
  const uint32_t r = db_len - h - (nblk - 2) * h, ro = r >> 2, bs = r & 3;
  uint32_t c[2 * HW + 1];
#pragma unroll
  for (int t = 0; t < HW; t++) c[t] = prev[t], c[HW + t] = cur[t];
  c[2 * HW] = 0;
#pragma unroll
  for (int s = 1; s <= HW; s <<= 1) {
    const bool on = (ro & s) != 0;
#pragma unroll
    for (int i = 0; i <= 2 * HW; i++) c[i] = on ? (i + s <= 2 * HW ? c[i + s] : 0u) : c[i];
  }
  // M' = 00 x 8 || H(msg) || salt, padded: 8 + 2 h bytes
  constexpr int NB = (2 + 2 * HW + 1 + BW / 8 + BW - 1) / BW;   // blocks with the 0x80 word and the length field
  uint32_t fw[NB * BW];
#pragma unroll
  for (int t = 0; t < NB * BW; t++) fw[t] = 0;
  {
    uint32_t shi = mw(2 * HW);
#pragma unroll
    for (int t = 0; t < HW; t++) {
      const uint32_t lo = mw(2 * HW - 1 - t);
      const uint32_t masked = (shi << 24) | (lo >> 8);
      shi = lo;
      const uint32_t mask = (uint32_t)(((((uint64_t)c[t] << 32) | c[t + 1]) << (8 * bs)) >> 32);
      fw[2 + t] = mh[t];
      fw[2 + HW + t] = masked ^ mask;
    }
  }
  fw[2 + 2 * HW] = 0x80000000u;
  fw[NB * BW - 1] = 8 * (8 + 2 * h);
  typename P::word st[8];
  P::init(st);
#pragma unroll 1
  for (int bi = 0; bi < NB; bi++) {
    uint32_t blk[BW];
#pragma unroll
    for (int t = 0; t < BW; t++) blk[t] = (NB > 1 && bi) ? fw[(NB - 1) * BW + t] : fw[t];
    P::compress(st, blk);
  }
#pragma unroll
  for (int t = 0; t < HW; t++) bad = bad || P::out(st, t) != hp[t];
  return bad ? RSA_MISMATCH : RSA_OK;
}

// bytes of the digest chosen by a CESS_RSA_DIGEST_* selector (0: unknown)
CESS_HD uint32_t digest_len(int digest) { return digest == 0 ? 32u : digest == 1 ? 48u : digest == 2 ? 64u : 0u; }

// the same over m in memory (word j at m[j * stride]) and H(msg) as the digest
// kernels write it (bytes, 4-byte aligned)
CESS_HD uint8_t check_stored(const uint32_t* m, uint64_t stride, uint32_t mod_bits, uint32_t k, const uint32_t* mhash,
                             int digest) {
  const uint32_t nw = (k + 3) / 4;
  auto mw = [=](uint32_t j) { return j < nw ? m[(uint64_t)j * stride] : 0u; };
  uint32_t mh[16];
#pragma unroll
  for (int t = 0; t < 16; t++) mh[t] = t < (int)(digest_len(digest) / 4) ? __builtin_bswap32(mhash[t]) : 0u;
  if (digest == 0) {
    uint32_t a[8];
#pragma unroll
    for (int t = 0; t < 8; t++) a[t] = mh[t];
    return check<P256>(mw, mod_bits, k, a);
  }
  if (digest == rsa_digest512::kSha384) {
    uint32_t a[12];
#pragma unroll
    for (int t = 0; t < 12; t++) a[t] = mh[t];
    return check<P384>(mw, mod_bits, k, a);
  }
  if (digest == rsa_digest512::kSha512) return check<P512f>(mw, mod_bits, k, mh);
  return RSA_MISMATCH;
}

}  // namespace rsa_pss
