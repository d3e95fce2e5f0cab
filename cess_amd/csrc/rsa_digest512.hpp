// What is SHA-384's and SHA-512's own in the digest kernels (k_rsa_digest512.hip;
// ring's RSA_PKCS1_2048_8192_SHA384, _SHA512 and RSA_PKCS1_3072_8192_SHA384,
// and Ed25519): the DigestInfo prefixes, the initial values, the compression
// function over a 128-byte block given as 32 big-endian 32-bit stream words,
// and the hash description Sha512 that hands them to rsa_digest.hpp's message
// stream and k_rsa_digest.hpp's kernel body.  Shared by the kernel and the
// host builds of the same code (tests/hostemu/rsa_digest512_emu.cpp,
// ed25519_emu.cpp).  The two digests differ in the initial values and in how
// many of the 64 state bytes are output (FIPS 180-4 §5.3.4-5, §6.4-5).
#pragma once
#include <stdint.h>

#include "rsa_digest.hpp"

namespace rsa_digest512 {

constexpr int kSha384 = 1, kSha512 = 2;   // the `digest` selector (CESS_RSA_DIGEST_*)

// DigestInfo prefixes (RFC 8017 §9.2 note 1): T = prefix || H, 19 + 48 = 67 or 19 + 64 = 83 bytes
using rsa_digest::kPrefixLen;
CESS_CONST uint8_t kPrefix384[kPrefixLen] = {0x30, 0x41, 0x30, 0x0d, 0x06, 0x09, 0x60, 0x86, 0x48, 0x01,
                                             0x65, 0x03, 0x04, 0x02, 0x02, 0x05, 0x00, 0x04, 0x30};
CESS_CONST uint8_t kPrefix512[kPrefixLen] = {0x30, 0x51, 0x30, 0x0d, 0x06, 0x09, 0x60, 0x86, 0x48, 0x01,
                                             0x65, 0x03, 0x04, 0x02, 0x03, 0x05, 0x00, 0x04, 0x40};

CESS_CONST uint64_t SHA384_IV[8] = {0xcbbb9d5dc1059ed8ull, 0x629a292a367cd507ull, 0x9159015a3070dd17ull,
                                    0x152fecd8f70e5939ull, 0x67332667ffc00b31ull, 0x8eb44a8768581511ull,
                                    0xdb0c2e0d64f98fa7ull, 0x47b5481dbefa4fa4ull};
CESS_CONST uint64_t SHA512_IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                                    0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                                    0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
CESS_CONST uint64_t SHA512_K[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,
    0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,
    0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
    0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
    0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,
    0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
    0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
    0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
    0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
    0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,
    0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,
    0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,
    0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
    0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
    0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};

// 64-bit rotations and shifts on the 32-bit halves: each half of the result
// is one 32-bit funnel shift (v_alignbit_b32) of the two input halves, where a
// 64-bit shift pair and an OR would be three instructions, two of them 64-bit.
// n is a compile-time constant, 0 < n < 64, n != 32.  The device build names
// the instruction: from the portable form the compiler rebuilds 64-bit shifts
// (v_lshlrev_b64 plus moves) for the high halves.
CESS_HD uint32_t fshr32(uint32_t hi, uint32_t lo, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)n);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> n);
#endif
}
CESS_HD uint64_t rotr64(uint64_t x, int n) {
  uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  if (n > 32) {
    const uint32_t t = lo;
    lo = hi;
    hi = t;
    n -= 32;
  }
  return ((uint64_t)fshr32(lo, hi, n) << 32) | fshr32(hi, lo, n);
}
CESS_HD uint64_t shr64(uint64_t x, int n) {   // n < 32
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  return ((uint64_t)(hi >> n) << 32) | fshr32(hi, lo, n);
}

// Round j (mod 8) of the compression over the working variables v: the roles
// a..h move one slot down per round instead of the values moving up, so a
// round writes two slots (d += t1, h = t1 + t2) and 8 rounds restore the roles.
// kw = K[i] + W[i].
CESS_HD void sha512_round(uint64_t (&v)[8], int j, uint64_t kw) {
  const uint64_t a = v[(0 - j) & 7], b = v[(1 - j) & 7], c = v[(2 - j) & 7];
  const uint64_t e = v[(4 - j) & 7], f = v[(5 - j) & 7], g = v[(6 - j) & 7];
  const uint64_t S1 = rotr64(e, 14) ^ rotr64(e, 18) ^ rotr64(e, 41);
  const uint64_t ch = (e & f) ^ (~e & g);
  const uint64_t t1 = v[(7 - j) & 7] + S1 + ch + kw;
  const uint64_t S0 = rotr64(a, 28) ^ rotr64(a, 34) ^ rotr64(a, 39);
  const uint64_t mj = (a & b) ^ (a & c) ^ (b & c);
  v[(3 - j) & 7] += t1;
  v[(7 - j) & 7] = t1 + S0 + mj;
}

// One 128-byte block, given as 32 big-endian 32-bit stream words (word pair
// 2 i, 2 i + 1 is the 64-bit message word i).  Rounds 0..15 take the block's
// words; rounds 16..79 run as four passes of one 16-round body that first
// advances the 16-word schedule in place: the schedule and role indices are
// compile-time (everything stays in registers) and the constants of a pass are
// read at a pass-uniform address.
CESS_HD void sha512_compress(uint64_t (&st)[8], const uint32_t (&blk)[32]) {
  uint64_t w[16], v[8];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = ((uint64_t)blk[2 * i] << 32) | blk[2 * i + 1];
#pragma unroll
  for (int i = 0; i < 8; i++) v[i] = st[i];
#pragma unroll
  for (int j = 0; j < 16; j++) sha512_round(v, j, SHA512_K[j] + w[j]);
#pragma unroll 1
  for (int i0 = 16; i0 < 80; i0 += 16) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint64_t w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
      const uint64_t s0 = rotr64(w15, 1) ^ rotr64(w15, 8) ^ shr64(w15, 7);
      const uint64_t s1 = rotr64(w2, 19) ^ rotr64(w2, 61) ^ shr64(w2, 6);
      w[j] = w[j] + s0 + w[(j + 9) & 15] + s1;
      sha512_round(v, j, SHA512_K[i0 + j] + w[j]);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] += v[i];
}

struct Sha512 {   // SHA-384 and SHA-512 (FIPS 180-4 §6.4-5): 128-byte blocks, a 128-bit length field
  using word = uint64_t;
  static constexpr int kBlockBytes = 128, kLenBytes = 16;
  static CESS_HD word iv(int digest, int j) { return digest == kSha384 ? SHA384_IV[j] : SHA512_IV[j]; }
  static CESS_HD uint32_t digest_len(int digest) { return digest == kSha384 ? 48u : 64u; }
  static CESS_HD uint32_t prefix_byte(int digest, int j) { return digest == kSha384 ? kPrefix384[j] : kPrefix512[j]; }
  static CESS_HD void compress(word (&st)[8], const uint32_t (&blk)[32]) { sha512_compress(st, blk); }
};

}  // namespace rsa_digest512
