// Host build of the hashed RSA mode's message padding and word assembly
// (cess_amd/csrc/rsa_digest.hpp) for tests/test_rsa_sha256.py: the same
// aligned-dword fetch, funnel shift and padding as k_rsa_digest, one message
// at a time.
#include "../../cess_amd/csrc/rsa_digest.hpp"

// SHA-256 of buf[start .. start + len) into out32.  Returns the number of
// fetched dwords that lie outside [buf, buf + total) rounded out to dword
// boundaries (must be 0).
extern "C" int emu_rsa_digest(const uint8_t* buf, uint64_t total, uint64_t start, uint64_t len, uint8_t* out32) {
  using namespace rsa_digest;
  const uint64_t lo_ok = (uint64_t)buf & ~(uint64_t)3, hi_ok = ((uint64_t)buf + total + 3) & ~(uint64_t)3;
  int outside = 0;
  auto fetch = [&](const uint32_t* p) {
    if ((uint64_t)p < lo_ok || (uint64_t)p + 4 > hi_ok) {
      outside++;
      return 0u;
    }
    return *p;
  };
  uint32_t st[8];
  for (int j = 0; j < 8; j++) st[j] = bls::SHA_IV[j];
  for (uint64_t pos0 = 0; pos0 < padded_len(len); pos0 += 64) {
    const uint32_t avail = window_avail(len, pos0);
    const uint64_t a0 = (uint64_t)buf + start + pos0;
    const uint32_t sh = (uint32_t)a0 & 3u;
    const uint32_t* base = reinterpret_cast<const uint32_t*>(a0 & ~(uint64_t)3);
    uint32_t blk[16];
    for (uint32_t j = 0; j < 16; j++) {
      const uint32_t lo = dword_needed(j, sh, avail) ? fetch(base + j) : 0xdeadbeefu;
      const uint32_t hi = dword_needed(j + 1, sh, avail) ? fetch(base + j + 1) : 0xdeadbeefu;
      blk[j] = stream_word(lo, hi, sh, avail, 4 * j, len, pos0);
    }
    bls::sha256_compress(st, blk);
  }
  for (int j = 0; j < 32; j++) out32[j] = (uint8_t)(st[j >> 2] >> (24 - 8 * (j & 3)));
  return outside;
}

// the last 64-byte block of the padded stream of a message of `len` bytes,
// with the message's own bytes as zeros (the padding function alone)
extern "C" void emu_rsa_digest_pad_block(uint64_t len, uint8_t* out64) {
  using namespace rsa_digest;
  const uint64_t p0 = padded_len(len) - 64;
  for (uint64_t j = 0; j < 16; j++) {
    const uint32_t w = pad_word_bytes(len, p0 + 4 * j);
    for (int q = 0; q < 4; q++) out64[4 * j + q] = (uint8_t)(w >> (24 - 8 * q));
  }
}

// the word form of the padding against the byte form over the message's last
// word and everything after it, and one block before and after that range;
// returns the number of words that differ
extern "C" int emu_rsa_digest_pad_word_check(uint64_t len) {
  using namespace rsa_digest;
  const uint64_t lo = (len & ~(uint64_t)3) > 64 ? (len & ~(uint64_t)3) - 64 : 0, hi = padded_len(len) + 64;
  int bad = 0;
  for (uint64_t p = lo; p < hi; p += 4) bad += pad_word(len, p) != pad_word_bytes(len, p);
  return bad;
}

extern "C" uint64_t emu_rsa_digest_padded_len(uint64_t len) { return rsa_digest::padded_len(len); }
