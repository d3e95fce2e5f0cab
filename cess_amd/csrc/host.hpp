// Internal declarations shared by the host translation units behind
// include/cess_bls.h (host.cpp: per-device context and the per-signature
// pipeline; host_rlc.cpp: RLC batch mode; host_multi.cpp: RCCL communicator,
// sharded batches and multi-device contexts; host_rsa.cpp: RSA batches;
// host_ed25519.cpp: Ed25519 batches; host_ed25519_sign.cpp: the Ed25519 signer;
// host_ecdsa.cpp: ECDSA P-256 batches;
// host_service.cpp: deserialize batch and verdict cache): the context, the
// entry-point and launch macros, the choice of the heavy kernels, message
// staging and the workers one file defines for another.  The index arithmetic
// that needs no HIP is in host_pure.hpp.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/cess_bls.h"
#include "../../include/cess_rsa.h"
#include "../../include/cess_ed25519.h"
#include "../../include/cess_ed25519_sign.h"
#include "../../include/cess_ecdsa.h"
#include "comm.hpp"
#include "host_pure.hpp"
#include "kernels.hpp"

// kernels (k_*.hip)
__global__ void k_decode_sig(uint64_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*, uint32_t*, uint64_t);
__global__ void k_decode_pk(uint64_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*, uint32_t*, uint64_t, uint32_t);
__global__ void k_hash(uint64_t, const uint8_t*, const uint64_t*, const uint8_t*, uint32_t*, uint64_t);
__global__ void k_prepare(uint64_t, const uint32_t*, uint4*, uint64_t, uint8_t*, const uint8_t*);
__global__ void k_norm_lines(uint4*);
__global__ void k_miller(uint64_t, const uint8_t*, const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*,
                         const uint4*, uint4*, uint4*, uint64_t, const uint32_t*, uint64_t, const uint8_t*);
__global__ void k_miller2(uint64_t, const uint8_t*, const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*,
                          const uint4*, uint4*, uint4*, uint64_t, const uint32_t*, uint64_t, const uint8_t*);
__global__ void k_miller_rr(uint64_t, uint64_t, const uint8_t*, const uint8_t*, const uint32_t*, const uint4*, uint4*,
                            uint64_t, uint64_t);
__global__ void k_miller_rr2(uint64_t, uint64_t, const uint8_t*, const uint8_t*, const uint32_t*, const uint4*, uint4*,
                            uint64_t, uint64_t);
__global__ void k_norm_keys(uint64_t, uint64_t, uint4*, uint32_t*, uint8_t*);
__global__ void k_merge_pk(uint64_t, const uint32_t*, uint32_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
__global__ void k_final(uint64_t, uint8_t*, uint4*, uint4*, uint64_t*, uint8_t*, uint64_t);
__global__ void k_final2(uint64_t, uint8_t*, uint4*, uint4*, uint64_t*, uint8_t*, uint64_t);
__global__ void k_keygen(uint64_t, const uint8_t*, uint8_t*);
__global__ void k_sign(uint64_t, const uint8_t*, const uint8_t*, const uint64_t*, uint8_t*);
__global__ void k_hash_out(uint64_t, const uint8_t*, const uint64_t*, uint8_t*);
// small-batch (latency) path (k_group.hip): one signature per wave
__global__ void k_group(uint64_t, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, const uint32_t*,
                        const uint32_t*, const uint32_t*, uint64_t, uint8_t*, uint8_t*);
__global__ void k_codes_bitmap(uint64_t, const uint8_t*, uint64_t*);
// digests of a batch's messages (k_rsa_digest.hpp; the hashed RSA mode's T_i = DigestInfo || H(msg_i) or the
// digests alone, Ed25519's SHA-512): SHA-256, and SHA-384 / SHA-512 by the last argument (CESS_RSA_DIGEST_*)
__global__ void k_rsa_digest(uint64_t, const uint8_t*, const uint64_t*, uint8_t*, uint32_t, uint64_t*);
__global__ void k_rsa_digest512(uint64_t, const uint8_t*, const uint64_t*, uint8_t*, uint32_t, uint64_t*, int);
// RLC batch mode (k_rlc.hip)
__global__ void k_rlc_scale(uint64_t, const uint8_t*, const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*,
                            uint64_t, uint32_t*, uint32_t*, uint64_t, uint64_t, uint32_t);
__global__ void k_rlcd_scale(uint64_t, const uint8_t*, const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*,
                            uint64_t, uint32_t*, uint32_t*, uint64_t, uint64_t);
__global__ void k_gt_prod(uint32_t, const uint8_t*, uint4*, uint8_t*);
__global__ void k_g1_sum_segs(uint32_t, const uint64_t*, const uint64_t*, const uint32_t*, const uint32_t*, uint64_t,
                              uint32_t*, uint64_t);
__global__ void k_rlc_pairs_list(uint32_t, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, const uint8_t*, uint8_t*,
                                 uint8_t*, uint32_t*, uint32_t*, const uint32_t*);
__global__ void k_fp12_prod_segs(uint32_t, const uint32_t*, const uint4*, uint64_t, uint4*, uint4*);
__global__ void k_rlcd_records(uint64_t, const uint8_t*, const uint8_t*, const uint32_t*, uint64_t, uint32_t*, uint8_t*,
                               uint64_t);
__global__ void k_rlcd_s_records(uint32_t, const uint32_t*, uint8_t*, uint8_t*, uint32_t*);
__global__ void k_fp12_prod_chunks(uint32_t, const uint64_t*, const uint64_t*, const uint8_t*, const uint4*, uint64_t,
                                   uint4*);
__global__ void k_fp12_mul_each(uint32_t, uint4*, const uint4*);
__global__ void k_group_fe(uint32_t, const uint4*, uint8_t*, uint8_t*);
__global__ void k_msm_count(uint64_t, const uint8_t*, const uint8_t*, MsmSegs, const uint32_t*, uint64_t, uint32_t*);
__global__ void k_msm_scatter(uint64_t, const uint8_t*, const uint8_t*, MsmSegs, const uint32_t*, uint64_t, uint32_t*,
                              uint32_t*);
__global__ void k_inv_perm(uint64_t, const uint32_t*, uint32_t*);
__global__ void k_msm_aos(uint64_t, const uint32_t*, uint4*);
__global__ void k_msm_items(uint32_t, uint32_t, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*,
                            const uint4*, const uint4*, uint32_t*, uint64_t);
__global__ void k_msm_bucket_sum(uint32_t, const uint32_t*, const uint32_t*, uint64_t, uint32_t*);
__global__ void k_msm_window(uint32_t, const uint32_t*, uint64_t, uint32_t*);
__global__ void k_msm_wsum(uint32_t, const uint32_t*, uint32_t*);
__global__ void k_msm_finish(uint32_t, uint32_t, const uint32_t*, uint32_t*, uint32_t*);

namespace cess_host {

enum Stage { ST_DECODE_SIG, ST_DECODE_PK, ST_HASH, ST_PREPARE, ST_MILLER, ST_FINAL, ST_RSA_CLASSIFY, ST_RSA_VERIFY,
             ST_GROUP, ST_SIGN, ST_RSA_DIGEST, ST_ED25519_KEYS, ST_ED25519_PACK, ST_ED25519_VERIFY,
             // the Ed25519 signer's (cess_ed25519_sign_stage_stats)
             ST_ED25519_COMB, ST_ED25519_SIGNERS, ST_ED25519_SIGN_PACK, ST_ED25519_SIGN_R, ST_ED25519_SIGN_S,
             // ECDSA P-256 (cess_ecdsa_stage_stats)
             ST_ECDSA_KEYS, ST_ECDSA_PACK, ST_ECDSA_VERIFY,
             // RSASSA-PSS's EM check (cess_rsa_pss_stage_stats): over the unsorted class lists, and over
             // the key-uniform ones, so that the stage tells which list path a call took
             ST_RSA_PSS, ST_RSA_PSS_U, ST_N };
constexpr int kBlock = 256;

inline unsigned grid_for(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int ensure(size_t want) {
    if (want <= bytes) return CESS_BLS_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    if (hipMalloc(&p, want) != hipSuccess) return CESS_BLS_E_OOM;
    bytes = want;
    return CESS_BLS_OK;
  }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

// State of one RLC batch between cess_bls_rlc_begin and cess_bls_rlc_finish.
struct RlcState {
  uint64_t n = 0;
  const uint8_t *sigs = nullptr, *pks = nullptr, *msgs = nullptr;   // caller's records (kept valid by the caller)
  const uint64_t* offs = nullptr;
  std::vector<uint8_t> codes;       // decode codes; 0 = candidate for the pairing check
  std::vector<uint32_t> perm;       // record indices sorted by key group
  std::vector<uint64_t> gbeg;       // K + 1 group boundaries in perm
  uint32_t K = 0;
  bool local_ok = false;
  // set only when the most recent rlc_begin completed: rlc_finish refuses
  // (CESS_BLS_E_INVALID_ARG) otherwise, so a failed or partial begin can never
  // be finished into "all verified" (fail closed)
  bool valid = false;
  bool per_sig = false;             // too many distinct keys for a combination: verified per signature
  uint64_t checks = 0, leaves = 0, leaf_sigs = 0;
  DevBuf P, Q, d_perm, d_seed, part, S, Qs, pk_in, pk_code, pk_inf, pk_aff, pk_coeffs, pk_usable;
  DevBuf rec_code, rec_inf, rec_sig, rec_h, rec_f, rec_f2, acc, slots, fin_code, fin_bm, gt, gts, tmp;
  DevBuf seg, part2, rec_coeffs, lists, d_gt_all;
  // distinct-key RLC (CESS_BLS_F_RLC_DISTINCT): every record's Miller value
  // f_i (stride n), the chunk-product ping-pong arrays and chunk bounds
  bool distinct = false;
  DevBuf d_rec_f, pr_a, pr_b, pr_lo, pr_hi;
  // bucket sums of the first check (k_msm_*): records' affine points and codes
  // for the whole batch (SoA stride n), group ids, bucket tables
  bool pts = false;                 // the batch's points are kept on the device (bucket sums possible)
  bool pq = false;                  // P, Q (per-record multiples) computed
  bool aos = false, have_pos = false;
  uint64_t index_hi = 0;            // scalar index base of this batch (rlc_begin_at)
  DevBuf Xs, Xh, Xsa, Xha, d_pos, m_bounds, d_code, d_inf, d_grp, m_cnt, m_start, m_cur, m_items, m_idx, m_part, m_bsum, m_T, m_U;
};

// Stage buffers of one in-flight pipeline part (SoA, stride = qcap).
struct StageSlot {
  DevBuf inf, sig_aff, h_aff, pk_aff, coeffs;
  // the per-record key buffers (19.6 KB of line coefficients per signature)
  // only with_key_buffers: keyed batches never allocate them
  int ensure(uint64_t qcap, bool with_key_buffers) {
    int r = inf.ensure(qcap) | sig_aff.ensure(qcap * CESS_W_G1 * 4) | h_aff.ensure(qcap * CESS_W_G1 * 4);
    if (with_key_buffers) r |= pk_aff.ensure(qcap * CESS_W_G2 * 4) | coeffs.ensure(qcap * (uint64_t)CESS_W_COEFFS * 4);
    return r ? CESS_BLS_E_OOM : CESS_BLS_OK;
  }
};

// One profiled kernel launch: [a, b] events on the launch's stream.
struct ProfRec {
  int stage;
  hipEvent_t a, b;
};

}  // namespace cess_host

struct RsaState;   // host_rsa.cpp
struct Ed25519State;   // host_ed25519.cpp
struct Ed25519SignState;   // host_ed25519_sign.cpp
struct EcdsaState;   // host_ecdsa.cpp

struct cess_bls_ctx {
  int device = 0;
  uint64_t cap = 0;    // records per host-API chunk (staging buffers)
  uint64_t qcap = 0;   // records per kernel launch (pipeline part; stage-buffer stride)
  uint64_t small = 0;  // batches of at most this many records take the lane-group path (k_group)
  uint32_t flags = 0;
  uint32_t mode = CESS_BLS_MODE_PER_SIG;
  hipStream_t stream = nullptr;
  // Pipeline (run_chunk): a chunk longer than qcap runs as parts; the light
  // kernels of part i+1 (decode, hash, prepare: no LDS, 128 VGPRs) run on
  // stream2 while k_miller of part i (one wave per SIMD: 144 KiB of LDS, 256
  // VGPRs) runs on the launch stream, so they share the CUs' issue slots.
  // Two stage slots alternate between parts.
  hipStream_t stream2 = nullptr;
  // small-batch path: the key decode (stream2) and hashing (stream3) run
  // beside the signature decode; the key decode's codes go to code2/inf2
  hipStream_t stream3 = nullptr;
  cess_host::DevBuf code2, inf2;
  hipEvent_t ev_start = nullptr, ev_light[2] = {}, ev_mill[2] = {};
  cess_host::StageSlot slot[2];
  cess_host::DevBuf pre, code, fval, fe_slots, bitmap, neg_g2;
  // staging for the host-buffer APIs
  cess_host::DevBuf in_sigs, in_pks, in_msgs, in_offs, out_gt, in_sks, out_bytes;
  // profiling: per-launch events (pool reused after each collect)
  std::vector<hipEvent_t> evpool;
  size_t evused = 0;
  std::vector<cess_host::ProfRec> prof;
  double stage_ms[cess_host::ST_N] = {};
  uint64_t stage_launches[cess_host::ST_N] = {};
  cess_host::RlcState* rlc = nullptr;
  // distinct-key table (cess_bls_keys_load): decoded keys + G2Prepared rows, stride = nkeys
  uint32_t nkeys = 0;
  cess_host::DevBuf key_in, key_code, key_inf, key_aff, key_coeffs, in_idx;
  // per key: 1 if its lines were normalised to c2 = 1 (k_norm_keys)
  cess_host::DevBuf key_norm;
  // ordering of successive calls on possibly different streams: every entry
  // point waits for the previous call's work (done_ev on last_stream)
  hipEvent_t done_ev = nullptr;
  hipStream_t last_stream = nullptr;
  bool pending = false;
  // one host thread at a time (the ABI contract); a second concurrent caller
  // gets CESS_BLS_E_BUSY instead of racing on the context buffers
  std::mutex busy;
  // communicator of the sharded entry points (comm.hpp): RCCL
  // (cess_bls_comm_init, one rank per process and GPU) or host shared memory
  // (cess_bls_comm_init_shm); owned
  cess_host::Transport* xport = nullptr;
  int nranks = 1, rank = 0;
  cess_host::DevBuf comm_buf, comm_words, comm_codes;
  // multi-device context (cess_bls_config.n_devices > 1): one sub-context per
  // device, batches sharded by index across them from host threads
  std::vector<cess_bls_ctx*> subs;
  // RSA PKCS#1 v1.5 key tables and staging (host_rsa.cpp)
  RsaState* rsa = nullptr;
  // Ed25519 key tables and staging (host_ed25519.cpp)
  Ed25519State* ed25519 = nullptr;
  // Ed25519 signer table, comb table and staging (host_ed25519_sign.cpp)
  Ed25519SignState* ed25519_sign = nullptr;
  // ECDSA P-256 key tables, G's table and staging (host_ecdsa.cpp)
  EcdsaState* ecdsa = nullptr;
};

#define HIPCHK(x)                                 \
  do {                                            \
    if ((x) != hipSuccess) return CESS_BLS_E_HIP; \
  } while (0)

// every locking entry point: a context, held by this thread alone
#define ENTRY(c)                           \
  if (!(c)) return CESS_BLS_E_INVALID_ARG; \
  CtxLock lock_(c);                        \
  if (!lock_.ok()) return CESS_BLS_E_BUSY

// One kernel launch of context `c` on stream strm, bracketed by a pair of
// HIP events under CESS_BLS_F_PROFILE (bench.py's rooflines take the kernels'
// durations from them); call_end collects the records.
#define LAUNCH(stage, strm, ...)                \
  do {                                          \
    hipEvent_t pa_;                             \
    int pr_ = prof_begin(c, strm, stage, &pa_); \
    if (pr_) return pr_;                        \
    hipLaunchKernelGGL(__VA_ARGS__);            \
    pr_ = prof_end(c, strm, stage, pa_);        \
    if (pr_) return pr_;                        \
  } while (0)

namespace cess_host {

// RAII guard for the one-thread-at-a-time contract
struct CtxLock {
  std::unique_lock<std::mutex> lk;
  explicit CtxLock(cess_bls_ctx* c) : lk(c->busy, std::try_to_lock) {}
  bool ok() const { return lk.owns_lock(); }
};

// make stream s wait for the previous call's work; called by every entry point
// before it enqueues anything (the context buffers are shared across calls)
int order_begin(cess_bls_ctx* c, hipStream_t s);
// record the end of this call's work on s
int order_end(cess_bls_ctx* c, hipStream_t s);

// profiling brackets around one launch on stream s (no-ops without CESS_BLS_F_PROFILE)
int prof_begin(cess_bls_ctx* c, hipStream_t s, int stage, hipEvent_t* a);
int prof_end(cess_bls_ctx* c, hipStream_t s, int stage, hipEvent_t a);
int run_chunk(cess_bls_ctx* c, hipStream_t s, uint64_t n, const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs,
              const uint64_t* offs, const uint8_t* pre, uint8_t* codes, uint64_t* bitmap, uint8_t* gt);
int verify_host(cess_bls_ctx* c, size_t n, const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs,
                const uint64_t* offs, const uint8_t* pre, uint8_t* codes_out, uint64_t* bitmap_out, uint8_t* gt_out);
int verify_var_host(cess_bls_ctx* c, size_t n, const uint8_t* sig_data, const uint64_t* sig_offsets,
                    const uint8_t* pk_data, const uint64_t* pk_offsets, const uint8_t* msgs, const uint64_t* msg_offsets,
                    uint8_t* codes_out, uint64_t* bitmap_out);
// End of an entry point's work on s: the call's profile records go into the
// stage totals and their events back to the pool, then order_end.  Without
// CESS_BLS_F_PROFILE this is order_end alone; with it, it waits for the
// context's streams, so callers that hand results back call it after the
// synchronisation they need anyway.
int call_end(cess_bls_ctx* c, hipStream_t s);

// Upload one staged message range (rebase_offsets, host_pure.hpp): bytes
// [first, first + bytes) of msgs into d_msgs, which is allocated `slack` bytes
// longer (at least one byte in all), and the rebased offsets into d_offs, on
// s.  `rebased` is the source of an asynchronous copy: the caller neither
// reuses nor frees it before it has synchronised s.
int upload_msgs(hipStream_t s, const uint8_t* msgs, uint64_t first, uint64_t bytes,
                const std::vector<uint64_t>& rebased, DevBuf& d_msgs, DevBuf& d_offs, uint64_t slack = 0);
// RLC (host_rlc.cpp)
int rlc_begin(cess_bls_ctx* c, size_t n, const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs,
              const uint64_t* offs, const uint8_t* seed32, uint8_t* gt_out);
// index_hi: added to every record index of the scalar derivation (shard k
// passes k << 40, so shards never share an r_i under one seed)
int rlc_begin_at(cess_bls_ctx* c, size_t n, const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs,
                 const uint64_t* offs, const uint8_t* seed32, uint64_t index_hi, uint8_t* gt_out);
int rlc_finish(cess_bls_ctx* c, uint8_t* codes_out, uint64_t* bitmap_out, uint64_t* stats4);
int gt_product_is_one(cess_bls_ctx* c, size_t m, const uint8_t* gts, bool gts_on_device, int* is_one);
int verify_rlc_host(cess_bls_ctx* c, size_t n, const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs,
                    const uint64_t* offs, const uint8_t* seed32, uint8_t* codes_out, uint64_t* bitmap_out,
                    uint64_t* stats4);
// OS randomness for RLC seeds drawn by the library (mode = RLC)
int os_random(uint8_t* out, size_t n);

// The heavy kernels.  Miller loop: k_miller2 (default: a lane pair per
// signature, 256-thread blocks of 128 signatures, two waves per SIMD;
// bls/pair.hpp) or k_miller (one lane per signature, one wave per SIMD), env
// CESS_BLS_MILLER = lane, read once per process.  Both take the same arguments
// and write the same fval rows; k_miller2 runs config[1]'s Miller loop in
// 129.8-130.0 ms per 1 M against 149.5-149.7 (same box,
// profiles/round6_c_sweep_miller_pair.txt).  The distinct-key RLC's
// k_miller_rr2 / k_miller_rr follow the same choice.
typedef void (*MillerKernel)(uint64_t, const uint8_t*, const uint8_t*, const uint32_t*, const uint32_t*,
                             const uint32_t*, const uint4*, uint4*, uint4*, uint64_t, const uint32_t*, uint64_t,
                             const uint8_t*);
typedef void (*MillerRrKernel)(uint64_t, uint64_t, const uint8_t*, const uint8_t*, const uint32_t*, const uint4*,
                               uint4*, uint64_t, uint64_t);
inline bool miller_pair() {
  static const bool v = [] {
    const char* e = getenv("CESS_BLS_MILLER");
    return !(e && strcmp(e, "lane") == 0);
  }();
  return v;
}
inline MillerKernel miller_kernel() { return miller_pair() ? k_miller2 : k_miller; }
inline MillerRrKernel miller_rr_kernel() { return miller_pair() ? k_miller_rr2 : k_miller_rr; }
// the lane-pair kernels: blocks of CESS_PAIR_THREADS / 2 signatures
constexpr uint64_t kPairSigs = CESS_PAIR_THREADS / 2;
// (covering whole 64-record bitmap words: k_final2 writes 32-bit halves, one per
// wave of 32 signatures, so both waves of a word must exist)
inline unsigned pair_grid(uint64_t m) {
  const uint64_t m64 = (m + 63) & ~63ull;
  return (unsigned)((m64 + kPairSigs - 1) / kPairSigs);
}
inline dim3 miller_grid(uint64_t m) { return dim3(miller_pair() ? pair_grid(m) : grid_for(m)); }
inline dim3 miller_block() { return dim3(miller_pair() ? CESS_PAIR_THREADS : kBlock); }

// The final-exponentiation kernel: k_final2 (default: a lane pair per
// signature, the accumulator in LDS; bls/pair_fe.hpp) or k_final (one lane per
// signature, accumulators in HBM), env CESS_BLS_FINAL = lane.  Same arguments
// and outputs; k_final2 137.4-138.2 against 142.1 ms per 1 M on one box, ~99
// against ~332 KB/sig counted traffic (profiles/round6_e_sweep_final_pair.txt).
typedef void (*FinalKernel)(uint64_t, uint8_t*, uint4*, uint4*, uint64_t*, uint8_t*, uint64_t);
inline bool final_pair() {
  static const bool v = [] {
    const char* e = getenv("CESS_BLS_FINAL");
    return !(e && strcmp(e, "lane") == 0);
  }();
  return v;
}
inline FinalKernel final_kernel() { return final_pair() ? k_final2 : k_final; }
inline dim3 final_grid(uint64_t m) { return dim3(final_pair() ? pair_grid(m) : grid_for(m)); }
inline dim3 final_block() { return dim3(final_pair() ? CESS_PAIR_THREADS : kBlock); }

}  // namespace cess_host

// Workers that one host file defines and another calls (not part of the C ABI).
// single-device forms of the multi-device entry points (host.cpp, host_rsa.cpp)
int cess_keys_load_one(cess_bls_ctx* c, size_t k, const uint8_t* pks, uint8_t* key_codes_out);
int cess_keyed_one(cess_bls_ctx* c, size_t n, const uint8_t* sigs, const uint32_t* key_idx, const uint8_t* msgs,
                   const uint64_t* offs, uint8_t* codes_out, uint64_t* bitmap_out);
int cess_gen_one(cess_bls_ctx* c, int kind, size_t n, const uint8_t* sks, const uint8_t* msgs, const uint64_t* offs,
                 uint8_t* out);
int cess_rsa_one(cess_bls_ctx* s, size_t n, const uint32_t* key_idx, const uint8_t* sigs, const uint64_t* soffs,
                 const uint8_t* msgs, const uint64_t* moffs, uint8_t* codes_out, uint64_t* bitmap_out);
int cess_rsa_digest_one(cess_bls_ctx* s, int digest, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                        const uint64_t* soffs, const uint8_t* msgs, const uint64_t* moffs, uint8_t* codes_out,
                        uint64_t* bitmap_out);
void cess_rsa_state_free(cess_bls_ctx* c);
int cess_ed25519_one(cess_bls_ctx* s, size_t n, const uint32_t* key_idx, const uint8_t* sigs, const uint64_t* soffs,
                     const uint8_t* msgs, const uint64_t* moffs, uint8_t* codes_out, uint64_t* bitmap_out);
void cess_ed25519_state_free(cess_bls_ctx* c);
int cess_ed25519_sign_one(cess_bls_ctx* s, size_t n, const uint32_t* signer_idx, const uint8_t* msgs,
                          const uint64_t* moffs, uint8_t* sigs_out, uint8_t* codes_out);
void cess_ed25519_sign_state_free(cess_bls_ctx* c);
int cess_ecdsa_one(cess_bls_ctx* s, int alg, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                   const uint64_t* soffs, const uint8_t* msgs, const uint64_t* moffs, uint8_t* codes_out,
                   uint64_t* bitmap_out);
void cess_ecdsa_state_free(cess_bls_ctx* c);
// one process, several GPUs (host_multi.cpp)
int cess_multi_create(const cess_bls_config* cfg, int ndev, cess_bls_ctx* c);
int cess_multi_verify(cess_bls_ctx* c, size_t n, const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs,
                      const uint64_t* offs, uint8_t* codes_out, uint64_t* bitmap_out, bool rlc, const uint8_t* seed32,
                      uint64_t* stats4);
int cess_multi_verify_var(cess_bls_ctx* c, size_t n, const uint8_t* sig_data, const uint64_t* sig_offsets,
                          const uint8_t* pk_data, const uint64_t* pk_offsets, const uint8_t* msgs,
                          const uint64_t* msg_offsets, uint8_t* codes_out, uint64_t* bitmap_out);
int cess_multi_keyed(cess_bls_ctx* c, size_t n, const uint8_t* sigs, const uint32_t* key_idx, const uint8_t* msgs,
                     const uint64_t* offs, uint8_t* codes_out, uint64_t* bitmap_out);
int cess_multi_keys_load(cess_bls_ctx* c, size_t k, const uint8_t* pks, uint8_t* key_codes_out);
int cess_multi_gen(cess_bls_ctx* c, int kind, size_t n, const uint8_t* sks, const uint8_t* msgs, const uint64_t* offs,
                   uint8_t* out);
int cess_multi_gt(cess_bls_ctx* c, size_t n, const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs,
                  const uint64_t* offs, uint8_t* codes_out, uint8_t* gt_out);
int cess_multi_rsa(cess_bls_ctx* c, size_t n, const uint32_t* key_idx, const uint8_t* sigs, const uint64_t* soffs,
                   const uint8_t* msgs, const uint64_t* moffs, uint8_t* codes_out, uint64_t* bitmap_out);
int cess_multi_rsa_digest(cess_bls_ctx* c, int digest, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                          const uint64_t* soffs, const uint8_t* msgs, const uint64_t* moffs, uint8_t* codes_out,
                          uint64_t* bitmap_out);
int cess_multi_ed25519(cess_bls_ctx* c, size_t n, const uint32_t* key_idx, const uint8_t* sigs, const uint64_t* soffs,
                       const uint8_t* msgs, const uint64_t* moffs, uint8_t* codes_out, uint64_t* bitmap_out);
int cess_multi_ed25519_sign(cess_bls_ctx* c, size_t n, const uint32_t* signer_idx, const uint8_t* msgs,
                            const uint64_t* moffs, uint8_t* sigs_out, uint8_t* codes_out);
int cess_multi_ecdsa(cess_bls_ctx* c, int alg, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                     const uint64_t* soffs, const uint8_t* msgs, const uint64_t* moffs, uint8_t* codes_out,
                     uint64_t* bitmap_out);
