/* Batch Ed25519 verification on the GPU, under the rules of ring's
 * `signature::ED25519` (CESS_ED25519_POLICY_RING).  Same library and context
 * as cess_bls.h and cess_rsa.h; return values are infrastructure status as
 * there (CESS_BLS_OK, CESS_BLS_E_*), per-record results are codes.
 *
 * The chain's TEE worker types are Ed25519: NodePublicKey is
 * sp_core::ed25519::Public and NodeSignature is [u8; 64].
 *
 * A record is (key, msg, sig).  Rules, in ring's order (every failure is ring's
 * Err(Unspecified); the codes are this library's):
 *   1. key length != 32: the key does not load; its records get KEY.
 *   2. signature length != 64: SIG_LEN.
 *   3. S = sig[32..64) little-endian must be < L = 2^252 +
 *      27742317777372353535851937790883648493, else SIG_RANGE.
 *   4. A from the key: y = the low 255 bits reduced mod p WITHOUT a canonical
 *      check (an encoding of y + p is accepted); x as in RFC 8032 5.1.3; no
 *      root: the key does not load, its records get KEY; if x's parity differs
 *      from bit 255, x is negated (x = 0 with the sign bit set is accepted: x
 *      stays 0).  No small-order check and no subgroup check.
 *   5. h = SHA-512(sig[0..32) || key bytes as given || msg), little-endian,
 *      reduced mod L.
 *   6. R' = [S]B - [h]A, encoded canonically; accept iff those 32 bytes equal
 *      sig[0..32), else MISMATCH.  R is never decoded, so a non-canonical R
 *      never matches.  The equation is cofactorless.
 * Precedence, first that applies: KEY for a key index outside the table or a
 * key that is not 32 bytes, SIG_LEN, SIG_RANGE, KEY for a key that does not
 * decode, MISMATCH.
 *
 * NOT the chain's verifier.  sp_io::crypto::ed25519_verify in the reference's
 * Substrate pin resolves to ed25519-zebra or ed25519-dalek 1.x.  Their sources
 * were not available to check; from general knowledge (ZIP 215, the dalek 1.x
 * source -- UNVERIFIED) zebra is cofactored and lenient on the encodings of R
 * and A, and dalek 1.x checks only the top bits of S, so it does not reject
 * every S >= L.  All of them agree
 * on signatures made by an honest signer and differ on crafted inputs only
 * (INTEGRATION.md).  Hence the `policy` argument: only
 * CESS_ED25519_POLICY_RING exists, any other value is CESS_BLS_E_INVALID_ARG,
 * and no node host function is wired to this API. */
#ifndef CESS_ED25519_H
#define CESS_ED25519_H

#include "cess_bls.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CESS_ED25519_POLICY_RING 0

enum cess_ed25519_code {
  CESS_ED25519_OK = 0,
  CESS_ED25519_SIG_LEN = 1,
  CESS_ED25519_SIG_RANGE = 2,
  CESS_ED25519_KEY = 3,
  CESS_ED25519_MISMATCH = 4
};

/* Load the context's Ed25519 key table: key j is bytes [key_offsets[j],
 * key_offsets[j + 1]) of `keys` (k + 1 non-decreasing offsets).  Each key is
 * decoded on the GPU and expanded to a 960-byte table.  key_status_out (may be
 * NULL) receives 0 or CESS_BLS_E_BAD_KEY per key; a key that does not load
 * stays in the table and its records get CESS_ED25519_KEY.  Replaces the
 * previous Ed25519 table; the BLS and RSA tables are not touched.  k = 0
 * empties the table. */
int cess_ed25519_keys_load(cess_bls_ctx* ctx, size_t k, const uint8_t* keys, const uint64_t* key_offsets, int policy,
                           int* key_status_out);

/* n records in host buffers: record i is key key_idx[i] of the table,
 * signature bytes [sig_offsets[i], sig_offsets[i + 1]) of `sigs`, message bytes
 * [msg_offsets[i], msg_offsets[i + 1]) of `msgs` (n + 1 non-decreasing offsets
 * each).  codes_out: n bytes; bitmap_out: (n + 63) / 64 words, bit i set iff
 * record i is OK, the bits past n zero.  Either may be NULL.  n = 0 returns
 * CESS_BLS_OK and touches nothing.  A context over several devices shards the
 * batch by index. */
int cess_ed25519_verify_batch(cess_bls_ctx* ctx, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                              const uint64_t* sig_offsets, const uint8_t* msgs, const uint64_t* msg_offsets,
                              uint8_t* codes_out, uint64_t* bitmap_out);

/* The same over device-resident records, enqueued on `stream` (NULL: the
 * context's): d_codes receives n bytes.  Single-device contexts only.  Read
 * bounds: the messages are first copied into a staging buffer of the context,
 * so nothing outside the ranges the offsets give is read: of d_msgs only bytes
 * [d_msg_offsets[0], d_msg_offsets[n]), and of d_sigs only the 64-byte
 * signatures.  The call reads d_msg_offsets[0] and d_msg_offsets[n] back (one
 * synchronisation of the stream) to size that buffer.  The caller's offsets
 * must be non-decreasing; a record whose message offsets are not hashes as
 * empty.  The copy into the staging buffer is made by one lane per record,
 * byte by byte: negligible for TEE-sized messages (0.85 ms per 2^20 messages of
 * 32 bytes), linear in the message length, so a caller with kilobyte messages
 * pays for it. */
int cess_ed25519_verify_batch_device(cess_bls_ctx* ctx, size_t n, const uint32_t* d_key_idx, const uint8_t* d_sigs,
                                     const uint64_t* d_sig_offsets, const uint8_t* d_msgs,
                                     const uint64_t* d_msg_offsets, uint8_t* d_codes, void* stream);

/* One record against a private one-key table (a loaded table survives the
 * call).  *ok_out = 1 iff the record verifies.  Returns CESS_BLS_E_BAD_KEY
 * where the key does not load (rules 1 and 4), whatever the signature. */
int cess_ed25519_verify(cess_bls_ctx* ctx, const uint8_t* key, size_t key_len, const uint8_t* msg, size_t msg_len,
                        const uint8_t* sig, size_t sig_len, int policy, int* ok_out);

/* Under CESS_BLS_F_PROFILE: the summed durations (ms) and launch counts of the
 * Ed25519 kernels since the last reset, under their kernel names
 * (k_ed25519_keys, k_ed25519_pack, k_ed25519_verify), as cess_bls_stage_stats
 * reports the BLS and RSA stages; the hashing of a batch is that list's
 * k_rsa_digest.  Fills at most `max` entries and returns the number of stages. */
int cess_ed25519_stage_stats(cess_bls_ctx* ctx, const char** names, double* ms, uint64_t* launches, int max, int reset);

#ifdef __cplusplus
}
#endif
#endif
