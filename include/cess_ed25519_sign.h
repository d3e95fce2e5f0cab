/* Batch Ed25519 key derivation and signing on the GPU, under the rules of ring's
 * `Ed25519KeyPair` (from_seed_unchecked, from_seed_and_public_key, sign in
 * ed25519/signing.rs).  Same library and context as cess_bls.h, cess_rsa.h and
 * cess_ed25519.h; return values are infrastructure status as there
 * (CESS_BLS_OK, CESS_BLS_E_*), per-record results are codes.
 *
 * Key pair from a seed:
 *   h = SHA-512(seed); a = h[0..32) little-endian, clamped (bits 0, 1, 2 and 255
 *   cleared, bit 254 set); prefix = h[32..64); A = encode([a]B).  A seed that is
 *   not 32 bytes is ring's KeyRejected::invalid_encoding; with a public key
 *   given, a key that differs from A is inconsistent_components.
 * Signing:
 *   r = SHA-512(prefix || msg) mod L; R = encode([r]B);
 *   k = SHA-512(R || A || msg) mod L; S = (k a + r) mod L; the signature is
 *   R || S.  Deterministic: no randomness, no context or prehash variant, so
 *   the output equals ring's byte for byte.
 *
 * a mod L.  The table keeps a reduced mod L, not the clamped 255-bit integer.
 * The fixed-base multiplication recodes its scalar to signed radix-16 digits,
 * which is exact only below 2^256 * 7 / 15; a clamped scalar with high top bits
 * (about 9 seeds in 64) exceeds that, and the lost carry would give
 * [a - 2^256]B.  B has order L, so [a mod L]B = [a]B, and (k (a mod L) + r) mod L
 * is the same S.
 *
 * SIDE CHANNELS.  The rows of the multiplication table are addressed by the
 * digits of secret scalars (a at load time, the nonce r per record).  The
 * signer is NOT hardened against timing or cache observation by another
 * tenant of the device: the same standing as cess_bls_sign_batch.
 *
 * ZEROING.  The signer table (a, prefix), the nonce scalars and every staging
 * buffer of the context that held a seed, a prefix, a digest of either or a
 * nonce are zeroed with hipMemsetAsync on the call's stream before the call
 * ends, before they are replaced, and when the context is destroyed.  Host
 * memory of the caller is the caller's.
 *
 * SCOPE.  PKCS#8 parsing (from_pkcs8*) is host DER work and is not included;
 * neither are hedged nonces or Ed25519ph / Ed25519ctx. */
#ifndef CESS_ED25519_SIGN_H
#define CESS_ED25519_SIGN_H

#include "cess_bls.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-signer status of cess_ed25519_signers_load: the expected public key
 * differs from the one derived from the seed (ring: inconsistent_components) */
#define CESS_ED25519_E_INCONSISTENT (-12)

/* record codes of cess_ed25519_sign_batch */
#define CESS_ED25519_SIGN_OK 0
#define CESS_ED25519_SIGN_SIGNER 1 /* the index is outside the table or the signer did not load: 64 zero bytes */

/* Build the context's signer table: seed j is bytes [seed_offsets[j],
 * seed_offsets[j + 1]) of `seeds` (k + 1 non-decreasing offsets); a, prefix and
 * A of every signer are derived on the GPU.  expected_pubs (32 k bytes, may be
 * NULL): the key each seed must give.  pubs_out (32 k bytes, may be NULL)
 * receives A, zeros for a seed that is not 32 bytes.  status_out (k ints, may
 * be NULL): 0, CESS_BLS_E_BAD_KEY for a seed that is not 32 bytes,
 * CESS_ED25519_E_INCONSISTENT for a mismatch with expected_pubs[j].  A signer
 * that does not load stays in the table and its records get
 * CESS_ED25519_SIGN_SIGNER.  Replaces (and zeroes) the previous signer table
 * and touches no other table; k = 0 empties it.  A context over several devices
 * loads the table on each. */
int cess_ed25519_signers_load(cess_bls_ctx* ctx, size_t k, const uint8_t* seeds, const uint64_t* seed_offsets,
                              const uint8_t* expected_pubs, uint8_t* pubs_out, int* status_out);

/* n records in host buffers: record i is signed by signer signer_idx[i] of the
 * table over message bytes [msg_offsets[i], msg_offsets[i + 1]) of `msgs`
 * (n + 1 non-decreasing offsets).  sigs_out: 64 n bytes; codes_out: n bytes, may
 * be NULL.  n = 0 returns CESS_BLS_OK and touches nothing.  A context over
 * several devices shards the batch by index. */
int cess_ed25519_sign_batch(cess_bls_ctx* ctx, size_t n, const uint32_t* signer_idx, const uint8_t* msgs,
                            const uint64_t* msg_offsets, uint8_t* sigs_out, uint8_t* codes_out);

/* The same over device-resident records, enqueued on `stream` (NULL: the
 * context's): d_sigs_out receives 64 n bytes, d_codes (may be NULL) n bytes.
 * Single-device contexts only.  Ordering and read bounds as
 * cess_ed25519_verify_batch_device: the messages are copied into a staging
 * buffer of the context, so of d_msgs only bytes [d_msg_offsets[0],
 * d_msg_offsets[n]) are read; the call reads those two offsets back (one
 * synchronisation of the stream) to size that buffer and is otherwise only
 * enqueued; the offsets must be non-decreasing, and a record whose offsets are
 * not signs the empty message. */
int cess_ed25519_sign_batch_device(cess_bls_ctx* ctx, size_t n, const uint32_t* d_signer_idx, const uint8_t* d_msgs,
                                   const uint64_t* d_msg_offsets, uint8_t* d_sigs_out, uint8_t* d_codes, void* stream);

/* One record against a private one-signer table, which is zeroed before the
 * call returns (a loaded table survives the call).  sig_out64: 64 bytes;
 * pub_out32 (may be NULL): A.  Returns CESS_BLS_E_BAD_KEY for a seed that is
 * not 32 bytes. */
int cess_ed25519_sign(cess_bls_ctx* ctx, const uint8_t* seed, size_t seed_len, const uint8_t* msg, size_t msg_len,
                      uint8_t* sig_out64, uint8_t* pub_out32);

/* Under CESS_BLS_F_PROFILE: the summed durations (ms) and launch counts of the
 * signer's kernels since the last reset, under their kernel names
 * (k_ed25519_comb, k_ed25519_signers, k_ed25519_sign_pack, k_ed25519_sign_r,
 * k_ed25519_sign_s), in the shape of cess_ed25519_stage_stats; the hashing is
 * cess_bls_stage_stats' k_rsa_digest (one launch per signer load, two per
 * batch).  Fills at most `max` entries and returns the number of stages. */
int cess_ed25519_sign_stage_stats(cess_bls_ctx* ctx, const char** names, double* ms, uint64_t* launches, int max,
                                  int reset);

#ifdef __cplusplus
}
#endif
#endif
