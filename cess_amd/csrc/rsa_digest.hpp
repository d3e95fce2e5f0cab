// SHA-2 of variable-length, arbitrarily aligned messages for the hashed RSA
// mode (RSASSA-PKCS1-v1_5 with SHA-256, SHA-384 or SHA-512) and Ed25519
// (k_rsa_digest.hpp): the padded stream of a message as a pure function of
// (len, position), and the assembly of one big-endian 32-bit stream word from
// the two aligned little-endian dwords that hold its bytes.  Both are written
// once over a hash description H -- Sha256 below, rsa_digest512.hpp's Sha512 --
// that gives the stream's two constants (kBlockBytes, kLenBytes) and the hash
// itself: the state word type, iv(digest, j), digest_len(digest),
// prefix_byte(digest, j) and compress(st, blk) over a block of kBlockBytes / 4
// stream words (`digest` selects among the digests that share a compression).
// Shared by the kernels and the host build of the same code
// (tests/hostemu/rsa_digest_emu.hpp), which checks it for lengths no GPU test
// can afford.
//
// Loads.  The bytes of a message are only ever fetched as whole aligned
// dwords, and a dword is fetched only if it holds at least one byte of the
// message (dword_needed).  So the kernel reads nothing outside
// [msgs, msgs + msg_offs[n]) rounded out to dword boundaries: at most 3 bytes
// before msgs (only if msgs itself is not 4-byte aligned) and at most 3 bytes
// after the last message byte, all inside dwords that also hold message
// bytes.  An aligned dword never crosses a page, so any readable allocation
// satisfies this; the host staging buffer carries 4 spare bytes regardless.
#pragma once
#include <stdint.h>

#include "bls/h2c.hpp"

namespace rsa_digest {

// DigestInfo prefix of SHA-256 (RFC 8017 §9.2 note 1): T = kPrefix || H; all
// three SHA-2 DigestInfo prefixes are 19 bytes
constexpr int kPrefixLen = 19;
CESS_CONST uint8_t kPrefix[kPrefixLen] = {0x30, 0x31, 0x30, 0x0d, 0x06, 0x09, 0x60, 0x86, 0x48, 0x01,
                                          0x65, 0x03, 0x04, 0x02, 0x01, 0x05, 0x00, 0x04, 0x20};

struct Sha256 {   // FIPS 180-4 §6.2; the compression is bls/h2c.hpp's
  using word = uint32_t;
  static constexpr int kBlockBytes = 64, kLenBytes = 8;
  static CESS_HD word iv(int, int j) { return bls::SHA_IV[j]; }
  static CESS_HD uint32_t digest_len(int) { return 32; }
  static CESS_HD uint32_t prefix_byte(int, int j) { return kPrefix[j]; }
  static CESS_HD void compress(word (&st)[8], const uint32_t (&blk)[16]) { bls::sha256_compress(st, blk); }
};

// bytes of the padded stream: msg || 0x80 || 0.. || big-endian bit length of kLenBytes
template <class H>
CESS_HD uint64_t padded_len(uint64_t len) {
  return (len + 1 + H::kLenBytes + H::kBlockBytes - 1) & ~(uint64_t)(H::kBlockBytes - 1);
}

// byte `pos` of the padded stream for pos >= len (0 for pos < len: the
// message's own bytes are not this function's)
template <class H>
CESS_HD uint32_t pad_byte(uint64_t len, uint64_t pos) {
  if (pos < len) return 0;
  if (pos == len) return 0x80;
  const uint64_t end = padded_len<H>(len);
  if (pos >= end - 8 && pos < end) {
    // the low 64 bits of the bit length 8 len: all of it for len < 2^61 bytes,
    // the bound of these functions (a 128-bit length field's high 64 bits are zero)
    const uint64_t q = end - 1 - pos;   // 0 = least significant byte
    return (uint32_t)((len << 3) >> (8 * q)) & 0xff;
  }
  return 0;
}

// big-endian word of the padding bytes at stream positions p .. p + 3, byte by byte
template <class H>
CESS_HD uint32_t pad_word_bytes(uint64_t len, uint64_t p) {
  return (pad_byte<H>(len, p) << 24) | (pad_byte<H>(len, p + 1) << 16) | (pad_byte<H>(len, p + 2) << 8) |
         pad_byte<H>(len, p + 3);
}

// the same word for p a multiple of 4 (what the kernel asks for), without the
// per-byte branches: the 0x80 marker if it falls in this word, and the halves
// of len << 3 in the stream's last two words, which are whole words because
// the stream ends on a multiple of the block (the host build checks it against
// pad_word_bytes)
template <class H>
CESS_HD uint32_t pad_word(uint64_t len, uint64_t p) {
  const uint64_t end = padded_len<H>(len), bits = len << 3;
  uint32_t w = (len >= p && len - p < 4) ? 0x80000000u >> (8 * (uint32_t)(len - p)) : 0u;
  w |= p + 8 == end ? (uint32_t)(bits >> 32) : 0u;
  w |= p + 4 == end ? (uint32_t)bits : 0u;
  return w;
}

// A window of the stream starts at position pos0 (a multiple of the block);
// avail = window_avail(len, pos0) message bytes lie at or after pos0 (clamped,
// so the per-word tests below are 32-bit), the first of them at byte address
// a0 (sh = a0 & 3).  Aligned dword j (byte address (a0 & ~3) + 4 j) holds one
// of them iff 4 j < sh + avail.
constexpr uint32_t kWindowMax = 1u << 20;   // no window is longer
CESS_HD uint32_t window_avail(uint64_t len, uint64_t pos0) {
  if (len <= pos0) return 0;
  const uint64_t a = len - pos0;
  return a > kWindowMax ? kWindowMax : (uint32_t)a;
}
CESS_HD bool dword_needed(uint32_t j, uint32_t sh, uint32_t avail) { return avail != 0 && 4 * j < sh + avail; }

// Big-endian word of the padded stream at position pos0 + off (off a multiple
// of 4, off + 4 <= kWindowMax) of a message of `len` bytes.  lo / hi: the
// aligned little-endian dwords at (a & ~3) and (a & ~3) + 4 for a = a0 + off
// (any value where dword_needed says the dword holds no message byte).
template <class H>
CESS_HD uint32_t stream_word(uint32_t lo, uint32_t hi, uint32_t sh, uint32_t avail, uint32_t off, uint64_t len,
                             uint64_t pos0) {
  const uint32_t le = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));   // message bytes off .. off + 3
  const uint32_t be = __builtin_bswap32(le);
  if (off + 4 <= avail) return be;
  const uint32_t cnt = avail > off ? avail - off : 0;   // 0 .. 3 message bytes in this word
  const uint32_t keep = cnt ? ~(0xffffffffu >> (8 * cnt)) : 0u;
  return (be & keep) | pad_word<H>(len, pos0 + off);
}

}  // namespace rsa_digest
