// Host build of the hashed RSA mode's SHA-384 / SHA-512 padding, word assembly
// and compression (cess_amd/csrc/rsa_digest512.hpp) for tests/test_rsa_sha2.py:
// the same aligned-dword fetch, funnel shift and padding as k_rsa_digest512,
// one message at a time.
#include "../../cess_amd/csrc/rsa_digest512.hpp"

// SHA-384 (digest = 1) or SHA-512 (digest = 2) of buf[start .. start + len)
// into out (48 / 64 bytes).  Returns the number of fetched dwords that lie
// outside [buf, buf + total) rounded out to dword boundaries (must be 0).
extern "C" int emu_rsa_digest512(int digest, const uint8_t* buf, uint64_t total, uint64_t start, uint64_t len,
                                 uint8_t* out) {
  using namespace rsa_digest;
  using namespace rsa_digest512;
  const uint64_t lo_ok = (uint64_t)buf & ~(uint64_t)3, hi_ok = ((uint64_t)buf + total + 3) & ~(uint64_t)3;
  int outside = 0;
  auto fetch = [&](const uint32_t* p) {
    if ((uint64_t)p < lo_ok || (uint64_t)p + 4 > hi_ok) {
      outside++;
      return 0u;
    }
    return *p;
  };
  uint64_t st[8];
  for (int j = 0; j < 8; j++) st[j] = digest == kSha384 ? SHA384_IV[j] : SHA512_IV[j];
  for (uint64_t pos0 = 0; pos0 < padded_len512(len); pos0 += 128) {
    const uint32_t avail = window_avail(len, pos0);
    const uint64_t a0 = (uint64_t)buf + start + pos0;
    const uint32_t sh = (uint32_t)a0 & 3u;
    const uint32_t* base = reinterpret_cast<const uint32_t*>(a0 & ~(uint64_t)3);
    uint32_t blk[32];
    for (uint32_t j = 0; j < 32; j++) {
      const uint32_t lo = dword_needed(j, sh, avail) ? fetch(base + j) : 0xdeadbeefu;
      const uint32_t hi = dword_needed(j + 1, sh, avail) ? fetch(base + j + 1) : 0xdeadbeefu;
      blk[j] = stream_word512(lo, hi, sh, avail, 4 * j, len, pos0);
    }
    sha512_compress(st, blk);
  }
  for (uint32_t j = 0; j < digest_len(digest); j++) out[j] = (uint8_t)(st[j >> 3] >> (56 - 8 * (j & 7)));
  return outside;
}

// the last 128-byte block of the padded stream of a message of `len` bytes,
// with the message's own bytes as zeros (the padding function alone)
extern "C" void emu_rsa_digest512_pad_block(uint64_t len, uint8_t* out128) {
  using namespace rsa_digest512;
  const uint64_t p0 = padded_len512(len) - 128;
  for (uint64_t j = 0; j < 32; j++) {
    const uint32_t w = pad_word512_bytes(len, p0 + 4 * j);
    for (int q = 0; q < 4; q++) out128[4 * j + q] = (uint8_t)(w >> (24 - 8 * q));
  }
}

// the word form of the padding against the byte form over the message's last
// word and everything after it, and one block before and after that range;
// returns the number of words that differ
extern "C" int emu_rsa_digest512_pad_word_check(uint64_t len) {
  using namespace rsa_digest512;
  const uint64_t lo = (len & ~(uint64_t)3) > 128 ? (len & ~(uint64_t)3) - 128 : 0, hi = padded_len512(len) + 128;
  int bad = 0;
  for (uint64_t p = lo; p < hi; p += 4) bad += pad_word512(len, p) != pad_word512_bytes(len, p);
  return bad;
}

extern "C" uint64_t emu_rsa_digest512_padded_len(uint64_t len) { return rsa_digest512::padded_len512(len); }

// the DigestInfo prefix the kernel writes (19 bytes)
extern "C" void emu_rsa_digest512_prefix(int digest, uint8_t* out19) {
  for (int j = 0; j < rsa_digest512::kPrefixLen; j++) out19[j] = (uint8_t)rsa_digest512::prefix_byte(digest, j);
}
