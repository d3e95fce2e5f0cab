/* Driver of the Ed25519 oracle (oracle/ring_ed25519_ref.py links it with the
 * reference's third_party/fiat/curve25519.c and crypto/mem.c into
 * oracle/_ref/libring_ed25519.so).  TEST INFRASTRUCTURE ONLY.
 *
 * What is ring's own C here (called, never restated):
 *   GFp_x25519_ge_frombytes_vartime          the key's decoding
 *   GFp_x25519_sc_reduce                     the 64-byte digest mod L
 *   GFp_x25519_ge_double_scalarmult_vartime  [h](-A) + [S]B
 *   GFp_x25519_fe_invert, _fe_mul_ttt, _fe_tobytes, _fe_isnegative, _fe_neg
 *                                            the encoding of the result
 * What is this project's restatement of ring's Rust (ed25519/verification.rs,
 * scalar.rs from_bytes_checked, ops.rs invert_vartime and encode_point):
 *   the lengths; S compared with L; the negation of X and T; the order of the
 *   calls; the sign bit put into byte 31; the comparison of 32 bytes; and the
 *   mapping of ring's single error onto the codes of include/cess_ed25519.h
 *   with that header's precedence.
 * SHA-512 is the caller's (hashlib): no hash code of the reference is built.
 * The point structs come from the reference's header through #include. */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "third_party/fiat/internal.h"

int GFp_x25519_ge_frombytes_vartime(ge_p3 *h, const uint8_t s[32]);
void GFp_x25519_sc_reduce(uint8_t s[64]);
void GFp_x25519_ge_double_scalarmult_vartime(ge_p2 *r, const uint8_t *a, const ge_p3 *A, const uint8_t *b);
void GFp_x25519_fe_invert(fe *out, const fe *z);
void GFp_x25519_fe_mul_ttt(fe *h, const fe *f, const fe *g);
void GFp_x25519_fe_tobytes(uint8_t s[32], const fe *h);
uint8_t GFp_x25519_fe_isnegative(const fe *f);
void GFp_x25519_fe_neg(fe *f);

enum { ED_OK = 0, ED_SIG_LEN = 1, ED_SIG_RANGE = 2, ED_KEY = 3, ED_MISMATCH = 4 };

/* L, little-endian */
static const uint8_t kOrder[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7,
                                   0xa2, 0xde, 0xf9, 0xde, 0x14, 0,    0,    0,    0,    0,    0,
                                   0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};

static int below_order(const uint8_t s[32]) {
  for (int i = 31; i >= 0; i--) {
    if (s[i] != kOrder[i]) return s[i] < kOrder[i];
  }
  return 0;
}

/* x / z and y / z as 32 bytes with x's parity in bit 255 (ops.rs encode_point) */
static void encode(uint8_t out[32], const fe *x, const fe *y, const fe *z) {
  fe recip, xz, yz;
  GFp_x25519_fe_invert(&recip, z);
  GFp_x25519_fe_mul_ttt(&xz, x, &recip);
  GFp_x25519_fe_mul_ttt(&yz, y, &recip);
  GFp_x25519_fe_tobytes(out, &yz);
  out[31] ^= (uint8_t)(GFp_x25519_fe_isnegative(&xz) << 7);
}

/* the record's code; digest = SHA-512(R || key || msg) */
int ring_ed_verify(const uint8_t *key, size_t key_len, const uint8_t *digest, const uint8_t *sig, size_t sig_len) {
  if (key_len != 32) return ED_KEY;
  if (sig_len != 64) return ED_SIG_LEN;
  if (!below_order(sig + 32)) return ED_SIG_RANGE;
  ge_p3 a;
  memset(&a, 0, sizeof(a));
  if (GFp_x25519_ge_frombytes_vartime(&a, key) != 1) return ED_KEY;
  GFp_x25519_fe_neg(&a.X);
  GFp_x25519_fe_neg(&a.T);
  uint8_t h[64];
  memcpy(h, digest, 64);
  GFp_x25519_sc_reduce(h);
  ge_p2 r;
  memset(&r, 0, sizeof(r));
  GFp_x25519_ge_double_scalarmult_vartime(&r, h, &a, sig + 32);
  uint8_t check[32];
  encode(check, &r.X, &r.Y, &r.Z);
  return memcmp(check, sig, 32) == 0 ? ED_OK : ED_MISMATCH;
}

/* out32 = in64 mod L */
void ring_ed_sc_reduce(const uint8_t *in64, uint8_t *out32) {
  uint8_t s[64];
  memcpy(s, in64, 64);
  GFp_x25519_sc_reduce(s);
  memcpy(out32, s, 32);
}

/* 1 and the canonical affine x and y (32 bytes each) if the key decodes, else 0 */
int ring_ed_decode(const uint8_t *key, uint8_t *x32, uint8_t *y32) {
  ge_p3 a;
  memset(&a, 0, sizeof(a));
  if (GFp_x25519_ge_frombytes_vartime(&a, key) != 1) return 0;
  fe recip, t;
  GFp_x25519_fe_invert(&recip, &a.Z);
  GFp_x25519_fe_mul_ttt(&t, &a.X, &recip);
  GFp_x25519_fe_tobytes(x32, &t);
  GFp_x25519_fe_mul_ttt(&t, &a.Y, &recip);
  GFp_x25519_fe_tobytes(y32, &t);
  return 1;
}
