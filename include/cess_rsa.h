/*
 * cess_rsa.h -- C ABI of the MI355X batch RSA PKCS#1 v1.5 (raw) verifier
 * (SURVEY §8(f) rank 4), in the same library and context as cess_bls.h.
 *
 * Replaces cp_enclave_verify::verify_rsa (reference
 * primitives/enclave-verify/src/lib.rs:221-228):
 *     let pk = rsa::RsaPublicKey::from_public_key_der(key).unwrap();
 *     pk.verify(Pkcs1v15Sign::new_raw(), msg, sig).is_ok()
 * (rsa 0.8.2, Cargo.lock:6538-6541: RFC 8017 RSASSA-PKCS1-v1_5-VERIFY with no
 * DigestInfo prefix: EM = 0x00 0x01 0xff..0xff 0x00 || msg).
 *
 * Per-signature codes: 0 OK, 1 SIG_LEN (len != k), 2 SIG_RANGE (s >= n),
 * 3 MSG_LEN (k < len(msg) + 11), 4 MISMATCH, 5 KEY (no such key / the key did
 * not load).  Codes 1..5 are the reference's `false`.  Every modulus size
 * the crate accepts (up to 4096 bits) is verified on the GPU: 1024/2048-bit
 * size classes expanded at compile time (Podr2Key is a 2048-bit key) and a
 * loop-form kernel for 2049..4096 bits.  Keys the reference accepts but the
 * GPU cannot verify -- even moduli, n < 3, SPKI AlgorithmIdentifier
 * parameters other than NULL -- report CESS_RSA_E_UNSUPPORTED, never
 * CESS_BLS_E_BAD_KEY: the verdict path for them is the caller's (the node
 * hook answers "unavailable" and the runtime's unchanged
 * cp_enclave_verify::verify_rsa decides), so a GPU node never
 * turns a key the rsa crate accepts into a rejection.  BAD_KEY means the
 * crate's from_public_key_der fails too (malformed DER, > 4096 bits, e out of
 * [2, 2^33 - 1]).  Return values are infrastructure status as in cess_bls.h.
 */
#ifndef CESS_RSA_H
#define CESS_RSA_H

#include "cess_bls.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CESS_RSA_E_UNSUPPORTED (-10) /* the key parses (the reference accepts it) but the GPU cannot verify it */

enum cess_rsa_code {
  CESS_RSA_OK = 0,
  CESS_RSA_SIG_LEN = 1,
  CESS_RSA_SIG_RANGE = 2,
  CESS_RSA_MSG_LEN = 3,
  CESS_RSA_MISMATCH = 4,
  CESS_RSA_KEY = 5
};

#define CESS_RSA_KEY_SPKI 0  /* SubjectPublicKeyInfo DER: what RsaPublicKey::from_public_key_der parses */
#define CESS_RSA_KEY_PKCS1 1 /* RSAPublicKey DER: Podr2Key = [u8; 270] (primitives/common/src/lib.rs:54) */

/* Host-side DER parse (the key checks of rsa 0.8: n <= 4096 bits,
 * 2 <= e <= 2^33 - 1).  n_out (may be NULL) receives the big-endian modulus
 * (*n_len bytes).  CESS_BLS_E_BAD_KEY where from_public_key_der fails.
 * This reports ONLY whether the reference crate parses the key: a key it
 * parses but the GPU kernels cannot verify (even or tiny modulus, SPKI
 * AlgorithmIdentifier parameters other than NULL) returns CESS_BLS_OK here and
 * CESS_RSA_E_UNSUPPORTED from cess_rsa_keys_load / cess_rsa_verify. */
int cess_rsa_parse_key(const uint8_t* der, size_t len, int format, uint8_t* n_out, size_t n_cap, size_t* n_len,
                       uint64_t* e_out);

/* Distinct-key table: k DER keys (key j = ders[der_offsets[j] .. [j+1]));
 * per key status (0, CESS_BLS_E_BAD_KEY, CESS_RSA_E_UNSUPPORTED) in
 * key_status_out (may be NULL).  Montgomery constants are precomputed once
 * per key.  Replaces the context's previous RSA table. */
int cess_rsa_keys_load(cess_bls_ctx* ctx, size_t k, const uint8_t* ders, const uint64_t* der_offsets, int format,
                       int* key_status_out);

/* verify_rsa over a batch: record i = (key key_idx[i], msg i, sig i), byte
 * ranges by offsets (n + 1 entries each).  codes_out (n) / bitmap_out
 * (ceil(n/64) words, bit = code 0) may be NULL.  Host buffers. */
int cess_rsa_verify_batch(cess_bls_ctx* ctx, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                          const uint64_t* sig_offsets, const uint8_t* msgs, const uint64_t* msg_offsets,
                          uint8_t* codes_out, uint64_t* bitmap_out);

/* Device-resident form (every pointer in HBM; offsets relative to d_sigs /
 * d_msgs); enqueued on `stream` (NULL: the context's), not synchronised. */
int cess_rsa_verify_batch_device(cess_bls_ctx* ctx, size_t n, const uint32_t* d_key_idx, const uint8_t* d_sigs,
                                 const uint64_t* d_sig_offsets, const uint8_t* d_msgs,
                                 const uint64_t* d_msg_offsets, uint8_t* d_codes, void* stream);

/* cp_enclave_verify::verify_rsa(key, msg, sig) drop-in: SPKI DER key;
 * CESS_BLS_E_BAD_KEY where from_public_key_der(key).unwrap() panics
 * (CESS_RSA_E_UNSUPPORTED for keys the GPU cannot verify, see above); else
 * *ok_out = the verdict. */
int cess_rsa_verify(cess_bls_ctx* ctx, const uint8_t* key_der, size_t key_len, const uint8_t* msg, size_t msg_len,
                    const uint8_t* sig, size_t sig_len, int* ok_out);

/* ---------------------------------------------------------------------------
 * Hashed mode: RSASSA-PKCS1-v1_5 with SHA-256 of a variable-length message,
 * hashed on the GPU (k_rsa_digest).  Replaces the signature check of
 * verify_miner_cert (reference primitives/enclave-verify/src/lib.rs:165-169):
 *     sig_cert.verify_signature(&webpki::RSA_PKCS1_2048_8192_SHA256,
 *                               report_json_raw, ias_sig)
 * Record i passes iff sig_i^e mod n = 00 01 ff..ff 00 || T_i with
 * T_i = DigestInfo(SHA-256) || SHA-256(msg_i) (51 bytes); everything after the
 * hashing is the raw path above, over T_i in place of the message.
 *
 * Key policy.  Which keys load is chosen per table:
 *   CESS_RSA_POLICY_RSA_CRATE       the rsa crate's checks (the raw mode's)
 *   CESS_RSA_POLICY_RING_2048_8192  ring's under RSA_PKCS1_2048_8192_SHA256:
 *     well-formed DER; the modulus length rounded up to whole bytes at least
 *     2048 bits and the exact length at most 8192 bits (ring rounds up, so a
 *     2041-bit modulus passes and a 2040-bit one does not); n odd; e odd;
 *     3 <= e <= 2^33 - 1.  A key that fails any of these is
 *     CESS_BLS_E_BAD_KEY.  A key that passes but is longer than 4096 bits is
 *     CESS_RSA_E_UNSUPPORTED: the caller's CPU path decides.
 * The policy governs key acceptance only: either verify mode runs over
 * whatever table is loaded.
 * ------------------------------------------------------------------------- */
#define CESS_RSA_POLICY_RSA_CRATE 0
#define CESS_RSA_POLICY_RING_2048_8192 1

/* cess_rsa_parse_key under `policy`: whether that policy accepts the key
 * (moduli up to 8192 bits = 1024 bytes under the ring policy). */
int cess_rsa_parse_key_policy(const uint8_t* der, size_t len, int format, int policy, uint8_t* n_out, size_t n_cap,
                              size_t* n_len, uint64_t* e_out);

/* cess_rsa_keys_load under `policy` (policy 0: identical to cess_rsa_keys_load). */
int cess_rsa_keys_load_policy(cess_bls_ctx* ctx, size_t k, const uint8_t* ders, const uint64_t* der_offsets,
                              int format, int policy, int* key_status_out);

/* Hashed verification over a batch; arguments as cess_rsa_verify_batch, msgs
 * of any length and alignment.  Codes are cess_rsa_code; CESS_RSA_MSG_LEN now
 * means k < 62 (no room for T), which a ring-policy table never produces.
 * Host buffers; multi-device contexts shard the batch by index. */
int cess_rsa_verify_sha256_batch(cess_bls_ctx* ctx, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                                 const uint64_t* sig_offsets, const uint8_t* msgs, const uint64_t* msg_offsets,
                                 uint8_t* codes_out, uint64_t* bitmap_out);

/* Device-resident form: pointers and stream as cess_rsa_verify_batch_device.
 * d_msg_offsets must be non-decreasing (a record whose range is not ordered
 * or ends past d_msg_offsets[n] is hashed as the empty message).  The kernel
 * fetches message bytes as whole aligned dwords, and only dwords that hold a
 * message byte: it may read up to 3 bytes before d_msgs (if d_msgs is not
 * 4-byte aligned) and up to 3 bytes past d_msgs + d_msg_offsets[n], never
 * beyond the aligned dword of the first / last byte, so any device allocation
 * that holds the messages is large enough. */
int cess_rsa_verify_sha256_batch_device(cess_bls_ctx* ctx, size_t n, const uint32_t* d_key_idx, const uint8_t* d_sigs,
                                        const uint64_t* d_sig_offsets, const uint8_t* d_msgs,
                                        const uint64_t* d_msg_offsets, uint8_t* d_codes, void* stream);

/* verify_signature(&RSA_PKCS1_2048_8192_SHA256, msg, sig) drop-in for one
 * record: ring policy, key in `format`.  CESS_BLS_E_BAD_KEY where ring rejects
 * the key, CESS_RSA_E_UNSUPPORTED where the GPU cannot verify it; else
 * *ok_out = the verdict. */
int cess_rsa_verify_sha256(cess_bls_ctx* ctx, const uint8_t* key_der, size_t key_len, int format, const uint8_t* msg,
                           size_t msg_len, const uint8_t* sig, size_t sig_len, int* ok_out);

/* SHA-256 of n messages (host buffers) -> out32 (32 n bytes): the hashed
 * mode's digest kernel alone, exposed for tests. */
int cess_sha256_batch(cess_bls_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* msg_offsets, uint8_t* out32);

/* ---------------------------------------------------------------------------
 * The other digests of verify_miner_cert's SUPPORTED_SIG_ALGS (reference
 * primitives/enclave-verify/src/lib.rs:87-93): RSASSA-PKCS1-v1_5 with SHA-384
 * and SHA-512, hashed on the GPU (k_rsa_digest512), and ring's 3072-bit key
 * floor.  T_i = DigestInfo(H) || H(msg_i) is 51 / 67 / 83 bytes for SHA-256 /
 * SHA-384 / SHA-512; everything after the hashing is the raw path, as above.
 *
 *   CESS_RSA_POLICY_RING_3072_8192  ring's key checks under
 *     RSA_PKCS1_3072_8192_SHA384: CESS_RSA_POLICY_RING_2048_8192 with a floor
 *     of 3072 bits, compared as ring does against the modulus length rounded
 *     up to whole bytes (a 3065-bit modulus passes, a 3064-bit one does not).
 *     Keys longer than 4096 bits that pass are CESS_RSA_E_UNSUPPORTED.
 * ------------------------------------------------------------------------- */
#define CESS_RSA_DIGEST_SHA256 0
#define CESS_RSA_DIGEST_SHA384 1
#define CESS_RSA_DIGEST_SHA512 2
#define CESS_RSA_POLICY_RING_3072_8192 2
/* the four entries of SUPPORTED_SIG_ALGS: digest + key policy */
#define CESS_RSA_ALG_2048_8192_SHA256 0
#define CESS_RSA_ALG_2048_8192_SHA384 1
#define CESS_RSA_ALG_2048_8192_SHA512 2
#define CESS_RSA_ALG_3072_8192_SHA384 3

/* cess_rsa_verify_sha256_batch with the digest chosen by `digest`
 * (CESS_RSA_DIGEST_*; an unknown value is CESS_BLS_E_INVALID_ARG; SHA256 is
 * cess_rsa_verify_sha256_batch itself).  CESS_RSA_MSG_LEN means
 * k < len(T) + 11: k < 62, 78 or 94.  Runs over whatever table is loaded. */
int cess_rsa_verify_digest_batch(cess_bls_ctx* ctx, int digest, size_t n, const uint32_t* key_idx,
                                 const uint8_t* sigs, const uint64_t* sig_offsets, const uint8_t* msgs,
                                 const uint64_t* msg_offsets, uint8_t* codes_out, uint64_t* bitmap_out);

/* Device-resident form: pointers, stream, the ordering of d_msg_offsets and
 * the read bounds exactly as cess_rsa_verify_sha256_batch_device: message
 * bytes are fetched as whole aligned dwords, and only dwords that hold a
 * message byte, so the kernel may read up to 3 bytes before d_msgs (if d_msgs
 * is not 4-byte aligned) and up to 3 bytes past d_msgs + d_msg_offsets[n],
 * never beyond the aligned dword of the first / last byte. */
int cess_rsa_verify_digest_batch_device(cess_bls_ctx* ctx, int digest, size_t n, const uint32_t* d_key_idx,
                                        const uint8_t* d_sigs, const uint64_t* d_sig_offsets, const uint8_t* d_msgs,
                                        const uint64_t* d_msg_offsets, uint8_t* d_codes, void* stream);

/* verify_signature(alg, msg, sig) drop-in for one record and one of the four
 * algorithms (CESS_RSA_ALG_*; an unknown value is CESS_BLS_E_INVALID_ARG;
 * alg 0 is cess_rsa_verify_sha256): the key, in `format`, is loaded under the
 * algorithm's key policy.  CESS_BLS_E_BAD_KEY where ring rejects the key,
 * CESS_RSA_E_UNSUPPORTED where the GPU cannot verify it; else *ok_out = the
 * verdict. */
int cess_rsa_verify_alg(cess_bls_ctx* ctx, int alg, const uint8_t* key_der, size_t key_len, int format,
                        const uint8_t* msg, size_t msg_len, const uint8_t* sig, size_t sig_len, int* ok_out);

/* H(msg_i) of n messages (host buffers) -> out (32 / 48 / 64 bytes per
 * record): the digest kernels alone, exposed for tests.  digest = SHA256 is
 * cess_sha256_batch. */
int cess_sha2_batch(cess_bls_ctx* ctx, int digest, size_t n, const uint8_t* msgs, const uint64_t* msg_offsets,
                    uint8_t* out);

/* ---------------------------------------------------------------------------
 * RSASSA-PSS: ring's RSA_PSS_2048_8192_SHA256 / _SHA384 / _SHA512 (webpki's
 * RSA_PSS_2048_8192_*_LEGACY_KEY), hashed and checked on the GPU.  Same
 * exponentiation, key table and digest kernels as above; the check after
 * m = s^e mod n is EMSA-PSS-VERIFY (k_rsa_pss) as ring does it
 * (utils/ring/src/rsa/padding.rs:307-487): MGF1 over the same digest H, and a
 * salt of exactly h = len(H) bytes -- a signature that RFC 8017 accepts with
 * any other salt length fails.  With k the byte length of n:
 *   len(sig) != k -> SIG_LEN;  s >= n -> SIG_RANGE;  then, all MISMATCH:
 *   em_len = ceil((mod_bits - 1) / 8); where 8 divides mod_bits - 1, the first
 *   byte of m must be 0 and EM is the rest; EM = maskedDB || H' || 0xbc;
 *   the bits of maskedDB[0] above mod_bits - 1 must be 0;
 *   DB = maskedDB xor MGF1(H', len) with those bits cleared must be
 *   00 .. 00 01 || salt (h bytes);  H(00 x 8 || H(msg) || salt) == H'.
 * ring also rejects s == 0; here 0^e = 0 has no 0xbc trailer, so that record
 * is MISMATCH as well.  Precedence: KEY, SIG_LEN, SIG_RANGE, MISMATCH;
 * CESS_RSA_MSG_LEN is never produced.
 * Key policy: CESS_RSA_POLICY_RING_2048_8192, unchanged (the one-record entry
 * loads the key under it; the batch entries run over whatever table is
 * loaded).  A key below ring's floor (byte length under 256, i.e. under 2041
 * bits) -- which only another policy lets into a table and which every ring
 * PSS algorithm rejects -- gives CESS_RSA_KEY for its records of the right
 * signature length (the front end has answered SIG_LEN for the others).
 * `digest` is CESS_RSA_DIGEST_*; an unknown value is CESS_BLS_E_INVALID_ARG.
 * The CESS_RSA_ALG_* numbering and cess_rsa_verify_alg do not cover PSS.
 * ------------------------------------------------------------------------- */

/* Arguments, codes_out / bitmap_out and multi-device sharding as
 * cess_rsa_verify_digest_batch.  Host buffers. */
int cess_rsa_verify_pss_batch(cess_bls_ctx* ctx, int digest, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                              const uint64_t* sig_offsets, const uint8_t* msgs, const uint64_t* msg_offsets,
                              uint8_t* codes_out, uint64_t* bitmap_out);

/* Device-resident form: pointers, stream, the ordering of d_msg_offsets and
 * the read bounds exactly as cess_rsa_verify_digest_batch_device (message
 * bytes are fetched as whole aligned dwords, and only dwords that hold a
 * message byte: up to 3 bytes before d_msgs if it is not 4-byte aligned and
 * up to 3 bytes past d_msgs + d_msg_offsets[n], never beyond the aligned dword
 * of the first / last byte). */
int cess_rsa_verify_pss_batch_device(cess_bls_ctx* ctx, int digest, size_t n, const uint32_t* d_key_idx,
                                     const uint8_t* d_sigs, const uint64_t* d_sig_offsets, const uint8_t* d_msgs,
                                     const uint64_t* d_msg_offsets, uint8_t* d_codes, void* stream);

/* verify_signature(&RSA_PSS_2048_8192_<digest>, msg, sig) drop-in for one
 * record: the key, in `format`, is loaded under CESS_RSA_POLICY_RING_2048_8192.
 * CESS_BLS_E_BAD_KEY where ring rejects the key, CESS_RSA_E_UNSUPPORTED where
 * the GPU cannot verify it (a modulus the loop-form size class does not hold:
 * above 4112 bits); else *ok_out = the verdict. */
int cess_rsa_verify_pss(cess_bls_ctx* ctx, int digest, const uint8_t* key_der, size_t key_len, int format,
                        const uint8_t* msg, size_t msg_len, const uint8_t* sig, size_t sig_len, int* ok_out);

/* The EM check alone, exposed for tests (like cess_sha2_batch): record i is
 * the message value m_i = ems[em_offsets[i] .. [i+1]) (big-endian, as
 * s^e mod n would be) of a modulus of mod_bits[i] <= 4112 bits (the largest
 * the loop-form size class holds), and
 * H(msg_i) = digests[h i .. h i + h).  codes_out (n): CESS_RSA_OK or
 * CESS_RSA_MISMATCH; an m_i that is not ceil(mod_bits[i] / 8) bytes long is a
 * MISMATCH (ring reads m to its end).  Host buffers. */
int cess_rsa_pss_em_batch(cess_bls_ctx* ctx, int digest, size_t n, const uint32_t* mod_bits, const uint8_t* ems,
                          const uint64_t* em_offsets, const uint8_t* digests, uint8_t* codes_out);

/* cess_bls_stage_stats for the stages that are RSASSA-PSS's own: the EM check
 * as "k_rsa_pss" when the call took the unsorted class lists and "k_rsa_pss_u"
 * when it took the key-uniform ones (either includes the launch that marks
 * 1024-bit-class records; the digest, classify and exponentiation launches are
 * counted under k_rsa_digest, k_rsa_classify and k_rsa_verify of
 * cess_bls_stage_stats). */
int cess_rsa_pss_stage_stats(cess_bls_ctx* ctx, const char** names, double* ms, uint64_t* launches, int max,
                             int reset);

#ifdef __cplusplus
}
#endif
#endif /* CESS_RSA_H */
