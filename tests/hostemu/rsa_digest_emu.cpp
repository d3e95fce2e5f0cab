// Host build of the hashed RSA mode's SHA-256 message padding and word
// assembly for tests/test_rsa_sha256.py: rsa_digest_emu.hpp over
// rsa_digest::Sha256, as k_rsa_digest instantiates the kernel body.
#include "rsa_digest_emu.hpp"

using H = rsa_digest::Sha256;

// SHA-256 of buf[start .. start + len) into out32; the count of dwords fetched outside the buffer's
extern "C" int emu_rsa_digest(const uint8_t* buf, uint64_t total, uint64_t start, uint64_t len, uint8_t* out32) {
  return rsa_digest_emu::hash<H>(0, buf, total, start, len, out32);
}
extern "C" void emu_rsa_digest_pad_block(uint64_t len, uint8_t* out64) { rsa_digest_emu::pad_block<H>(len, out64); }
extern "C" int emu_rsa_digest_pad_word_check(uint64_t len) { return rsa_digest_emu::pad_word_check<H>(len); }
extern "C" uint64_t emu_rsa_digest_padded_len(uint64_t len) { return rsa_digest::padded_len<H>(len); }
