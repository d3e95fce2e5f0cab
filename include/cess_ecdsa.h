/* Batch ECDSA P-256 verification on the GPU, under the rules of ring 0.16.9's
 * `signature::ECDSA_P256_SHA256_FIXED`, `ECDSA_P256_SHA256_ASN1` and
 * `ECDSA_P256_SHA384_ASN1` (the algorithms webpki hands ECDSA-signed
 * certificates to).  Same library and context as cess_bls.h, cess_rsa.h and
 * cess_ed25519.h; return values are infrastructure status as there
 * (CESS_BLS_OK, CESS_BLS_E_*), per-record results are codes.
 *
 * A record is (key, msg, sig) under one algorithm id.  Rules, read from ring's
 * ec/suite_b/ecdsa/verification.rs, digest_scalar.rs, ec/suite_b/public_key.rs
 * and io/der.rs (every failure is ring's Err(Unspecified); the codes are this
 * library's).  q is the field prime, n the group order:
 *   1. Key: exactly 65 bytes, the first 0x04; x and y big-endian, each in
 *      [0, q - 1] (zero is allowed); y^2 = x^3 - 3 x + b mod q.  Compressed and
 *      hybrid encodings do not exist here.  A key that fails does not load; all
 *      of its records get KEY.
 *   2. Signature split.  FIXED: exactly 64 bytes, r || s, big-endian.  ASN1:
 *      SEQUENCE { INTEGER r, INTEGER s } under ring's der.rs, nothing after the
 *      sequence and nothing after s inside it.  A tag whose low five bits are
 *      all ones is rejected.  A length is the short form, or 0x81 with a byte
 *      >= 128, or 0x82 with a value >= 256; anything else is rejected.  An
 *      INTEGER is non-empty and not negative, carries a leading 0x00 only when
 *      the next byte has its top bit set, and is not zero.  Any failure:
 *      SIG_FORMAT.
 *   3. r and s in [1, n - 1], else SIG_RANGE (a value with more than 32
 *      significant bytes falls here).
 *   4. e = the leftmost 32 bytes of SHA-256(msg), or of SHA-384(msg) for the
 *      SHA-384 algorithm, as a big-endian integer, minus n once if it is >= n.
 *      e may be zero.
 *   5. w = 1 / s mod n, u1 = e w, u2 = r w, R = u1 G + u2 Q.  R at infinity:
 *      MISMATCH.
 *   6. Accept iff x(R) = r (mod n), tested as ring does: r Z^2 = X, and if
 *      r < q - n also (r + n) Z^2 = X.  Anything else: MISMATCH.
 * Precedence, first that applies: KEY (a key index outside the table or a key
 * that did not load), SIG_FORMAT, SIG_RANGE, MISMATCH.
 *
 * No node host function is wired to this API.  Out of scope:
 * P-384; signing; a pre-hashed entry (ring keeps verify_digest private);
 * secp256k1 (sp_io::crypto::ecdsa_*, whose source is not in the reference
 * tree). */
#ifndef CESS_ECDSA_H
#define CESS_ECDSA_H

#include "cess_bls.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CESS_ECDSA_ALG_P256_SHA256_FIXED 0
#define CESS_ECDSA_ALG_P256_SHA256_ASN1 1
#define CESS_ECDSA_ALG_P256_SHA384_ASN1 2

enum cess_ecdsa_code {
  CESS_ECDSA_OK = 0,
  CESS_ECDSA_SIG_FORMAT = 1,
  CESS_ECDSA_SIG_RANGE = 2,
  CESS_ECDSA_KEY = 3,
  CESS_ECDSA_MISMATCH = 4
};

/* Load the context's ECDSA key table: key j is bytes [key_offsets[j],
 * key_offsets[j + 1]) of `keys` (k + 1 non-decreasing offsets).  Each key is
 * validated on the GPU (rule 1) and expanded to a 960-byte table.
 * key_status_out (may be NULL) receives 0 or CESS_BLS_E_BAD_KEY per key; a key
 * that does not load stays in the table and its records get CESS_ECDSA_KEY.
 * Replaces the previous ECDSA table; the BLS, RSA and Ed25519 tables are not
 * touched.  k = 0 empties the table. */
int cess_ecdsa_keys_load(cess_bls_ctx* ctx, size_t k, const uint8_t* keys, const uint64_t* key_offsets,
                         int* key_status_out);

/* n records in host buffers under algorithm `alg` (any other value than the
 * three ids: CESS_BLS_E_INVALID_ARG): record i is key key_idx[i] of the table,
 * signature bytes [sig_offsets[i], sig_offsets[i + 1]) of `sigs` (any length),
 * message bytes [msg_offsets[i], msg_offsets[i + 1]) of `msgs` (n + 1
 * non-decreasing offsets each).  codes_out: n bytes; bitmap_out: (n + 63) / 64
 * words, bit i set iff record i is OK, the bits past n zero.  Either may be
 * NULL.  n = 0 returns CESS_BLS_OK and touches nothing.  A context over
 * several devices shards the batch by index. */
int cess_ecdsa_verify_batch(cess_bls_ctx* ctx, int alg, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                            const uint64_t* sig_offsets, const uint8_t* msgs, const uint64_t* msg_offsets,
                            uint8_t* codes_out, uint64_t* bitmap_out);

/* The same over device-resident records, enqueued on `stream` (NULL: the
 * context's): d_codes receives n bytes.  Single-device contexts only.  Read
 * bounds: the messages are first copied into a staging buffer of the context,
 * so nothing outside the ranges the offsets give is read: of d_msgs only bytes
 * [d_msg_offsets[0], d_msg_offsets[n]), and of d_sigs only bytes
 * [d_sig_offsets[0], d_sig_offsets[n]).  The call reads d_msg_offsets[0] and
 * d_msg_offsets[n] back (one synchronisation of the stream) to size that
 * buffer.  The caller's offsets must be non-decreasing; a record whose message
 * offsets are not hashes as empty, and one whose signature offsets are not is
 * an empty signature.  The copy into the staging buffer is made by one lane
 * per record, byte by byte: negligible for short messages, linear in the
 * message length, so a caller with kilobyte messages pays for it. */
int cess_ecdsa_verify_batch_device(cess_bls_ctx* ctx, int alg, size_t n, const uint32_t* d_key_idx,
                                   const uint8_t* d_sigs, const uint64_t* d_sig_offsets, const uint8_t* d_msgs,
                                   const uint64_t* d_msg_offsets, uint8_t* d_codes, void* stream);

/* One record against a private one-key table (a loaded table survives the
 * call).  *ok_out = 1 iff the record verifies.  Returns CESS_BLS_E_BAD_KEY
 * where the key does not load (rule 1), whatever the signature. */
int cess_ecdsa_verify(cess_bls_ctx* ctx, int alg, const uint8_t* key, size_t key_len, const uint8_t* msg,
                      size_t msg_len, const uint8_t* sig, size_t sig_len, int* ok_out);

/* Under CESS_BLS_F_PROFILE: the summed durations (ms) and launch counts of the
 * ECDSA kernels since the last reset, under their kernel names (k_ecdsa_keys,
 * k_ecdsa_pack, k_ecdsa_verify), as cess_bls_stage_stats reports the BLS and
 * RSA stages; the hashing of a batch is that list's k_rsa_digest.  Fills at
 * most `max` entries and returns the number of stages. */
int cess_ecdsa_stage_stats(cess_bls_ctx* ctx, const char** names, double* ms, uint64_t* launches, int max, int reset);

#ifdef __cplusplus
}
#endif
#endif
