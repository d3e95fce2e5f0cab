// Host build of the digest kernels' message padding and word assembly
// (cess_amd/csrc/rsa_digest.hpp) over a hash description H, for
// rsa_digest_emu.cpp (SHA-256) and rsa_digest512_emu.cpp (SHA-384 / SHA-512):
// the same aligned-dword fetch, funnel shift and padding as the kernels, one
// message at a time.
#pragma once
#include "../../cess_amd/csrc/rsa_digest.hpp"

namespace rsa_digest_emu {

using namespace rsa_digest;

// H (selector `digest`) of buf[start .. start + len) into out (digest_len
// bytes).  Returns the number of fetched dwords that lie outside
// [buf, buf + total) rounded out to dword boundaries (must be 0).
template <class H>
int hash(int digest, const uint8_t* buf, uint64_t total, uint64_t start, uint64_t len, uint8_t* out) {
  constexpr uint32_t kBlock = H::kBlockBytes, kWords = kBlock / 4, kWordBytes = sizeof(typename H::word);
  const uint64_t lo_ok = (uint64_t)buf & ~(uint64_t)3, hi_ok = ((uint64_t)buf + total + 3) & ~(uint64_t)3;
  int outside = 0;
  auto fetch = [&](const uint32_t* p) {
    if ((uint64_t)p < lo_ok || (uint64_t)p + 4 > hi_ok) {
      outside++;
      return 0u;
    }
    return *p;
  };
  typename H::word st[8];
  for (int j = 0; j < 8; j++) st[j] = H::iv(digest, j);
  for (uint64_t pos0 = 0; pos0 < padded_len<H>(len); pos0 += kBlock) {
    const uint32_t avail = window_avail(len, pos0);
    const uint64_t a0 = (uint64_t)buf + start + pos0;
    const uint32_t sh = (uint32_t)a0 & 3u;
    const uint32_t* base = reinterpret_cast<const uint32_t*>(a0 & ~(uint64_t)3);
    uint32_t blk[kWords];
    for (uint32_t j = 0; j < kWords; j++) {
      const uint32_t lo = dword_needed(j, sh, avail) ? fetch(base + j) : 0xdeadbeefu;
      const uint32_t hi = dword_needed(j + 1, sh, avail) ? fetch(base + j + 1) : 0xdeadbeefu;
      blk[j] = stream_word<H>(lo, hi, sh, avail, 4 * j, len, pos0);
    }
    H::compress(st, blk);
  }
  for (uint32_t j = 0; j < H::digest_len(digest); j++)
    out[j] = (uint8_t)(st[j / kWordBytes] >> (8 * (kWordBytes - 1 - j % kWordBytes)));
  return outside;
}

// the last block of the padded stream of a message of `len` bytes, with the
// message's own bytes as zeros (the padding function alone)
template <class H>
void pad_block(uint64_t len, uint8_t* out) {
  const uint64_t p0 = padded_len<H>(len) - H::kBlockBytes;
  for (uint64_t j = 0; j < H::kBlockBytes / 4; j++) {
    const uint32_t w = pad_word_bytes<H>(len, p0 + 4 * j);
    for (int q = 0; q < 4; q++) out[4 * j + q] = (uint8_t)(w >> (24 - 8 * q));
  }
}

// the word form of the padding against the byte form over the message's last
// word and everything after it, and one block before and after that range;
// returns the number of words that differ
template <class H>
int pad_word_check(uint64_t len) {
  constexpr uint64_t kBlock = H::kBlockBytes;
  const uint64_t lo = (len & ~(uint64_t)3) > kBlock ? (len & ~(uint64_t)3) - kBlock : 0, hi = padded_len<H>(len) + kBlock;
  int bad = 0;
  for (uint64_t p = lo; p < hi; p += 4) bad += pad_word<H>(len, p) != pad_word_bytes<H>(len, p);
  return bad;
}

}  // namespace rsa_digest_emu
