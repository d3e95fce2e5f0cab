// Host build of the hashed RSA mode's SHA-384 / SHA-512 padding, word assembly
// and compression (cess_amd/csrc/rsa_digest512.hpp) for tests/test_rsa_sha2.py:
// rsa_digest_emu.hpp over rsa_digest512::Sha512, as k_rsa_digest512
// instantiates the kernel body.
#include "../../cess_amd/csrc/rsa_digest512.hpp"
#include "rsa_digest_emu.hpp"

using H = rsa_digest512::Sha512;

// SHA-384 (digest = 1) or SHA-512 (digest = 2) of buf[start .. start + len) into out (48 / 64 bytes);
// the count of dwords fetched outside the buffer's
extern "C" int emu_rsa_digest512(int digest, const uint8_t* buf, uint64_t total, uint64_t start, uint64_t len,
                                 uint8_t* out) {
  return rsa_digest_emu::hash<H>(digest, buf, total, start, len, out);
}
extern "C" void emu_rsa_digest512_pad_block(uint64_t len, uint8_t* out128) { rsa_digest_emu::pad_block<H>(len, out128); }
extern "C" int emu_rsa_digest512_pad_word_check(uint64_t len) { return rsa_digest_emu::pad_word_check<H>(len); }
extern "C" uint64_t emu_rsa_digest512_padded_len(uint64_t len) { return rsa_digest::padded_len<H>(len); }

// the DigestInfo prefix the kernel writes (19 bytes)
extern "C" void emu_rsa_digest512_prefix(int digest, uint8_t* out19) {
  for (int j = 0; j < rsa_digest512::kPrefixLen; j++) out19[j] = (uint8_t)H::prefix_byte(digest, j);
}
