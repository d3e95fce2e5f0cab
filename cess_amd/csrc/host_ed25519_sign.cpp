// Host side of the Ed25519 batch signer (include/cess_ed25519_sign.h): the comb
// table of the base point (k_ed25519_comb, once per context), the signer table
// (k_rsa_digest512 over the staged seeds, then k_ed25519_signers), and per batch
// the nonce input (k_ed25519_sign_pack), its digests, R (k_ed25519_sign_r), the
// second hash input (k_ed25519_sign_pack again), its digests and S
// (k_ed25519_sign_s).  Staging, launches and the call end are host.hpp's; the
// entry points have the shape of host_ed25519.cpp's.
//
// Zeroing: every device buffer that held a seed, a digest of a seed or of a
// nonce input, a prefix or a nonce is cleared with hipMemsetAsync on the call's
// stream before the call's end is recorded (wipe_staging); a signer table is
// cleared before it is replaced and when the context is destroyed.
#include "host.hpp"

#include "ed25519_sign.hpp"

using namespace cess_host;

__global__ void k_ed25519_comb(uint32_t*, uint8_t*);
__global__ void k_ed25519_signers(uint64_t, const uint32_t*, const uint64_t*, const uint8_t*, const uint8_t*, uint32_t*,
                                  uint32_t*, uint32_t*, uint8_t*);
__global__ void k_ed25519_sign_pack(uint64_t, const uint32_t*, uint32_t, const uint8_t*, const uint8_t*, const uint8_t*,
                                    const uint8_t*, const uint64_t*, uint8_t*, uint64_t*);
__global__ void k_ed25519_sign_r(uint64_t, const uint32_t*, uint32_t, const uint8_t*, const uint32_t*, const uint8_t*,
                                 uint32_t*, uint8_t*);
__global__ void k_ed25519_sign_s(uint64_t, const uint32_t*, uint32_t, const uint8_t*, const uint32_t*, const uint8_t*,
                                 const uint32_t*, uint8_t*, uint8_t*);

// per-context signer tables: the caller's and a one-signer table for cess_ed25519_sign
struct SignerTable {
  DevBuf a, prefix, pub, status;   // 32, 32, 32 and 1 bytes per signer
  uint32_t n = 0;
};
struct Ed25519SignState {
  SignerTable user, single;
  DevBuf comb, comb_status;        // the multiples of 16^i B, built once per context
  bool have_comb = false;
  DevBuf seed_in, seed_offs, seed_dig, expected;
  DevBuf in_idx, in_msgs, in_moffs, out_sigs, out_codes;
  DevBuf pack, pack_offs, digests, nonces;
};

static Ed25519SignState& sg_state(cess_bls_ctx* c) {
  if (!c->ed25519_sign) c->ed25519_sign = new Ed25519SignState();
  return *c->ed25519_sign;
}

static void wipe(DevBuf& b, hipStream_t s) {
  if (b.p) (void)hipMemsetAsync(b.p, 0, b.bytes, s);
}
static void wipe_table(SignerTable& T, hipStream_t s) {
  wipe(T.a, s);
  wipe(T.prefix, s);
  T.n = 0;
}
// the staging buffers that held secrets of a call; enqueued before the call's end is recorded
static void wipe_staging(Ed25519SignState& S, hipStream_t s) {
  for (DevBuf* b : {&S.seed_in, &S.seed_dig, &S.pack, &S.digests, &S.nonces}) wipe(*b, s);
}

void cess_ed25519_sign_state_free(cess_bls_ctx* c) {
  if (!c->ed25519_sign) return;
  // (the context's streams are gone: the null stream of its device, waited for before the buffers are freed)
  (void)hipSetDevice(c->device);
  Ed25519SignState& S = *c->ed25519_sign;
  wipe_table(S.user, nullptr);
  wipe_table(S.single, nullptr);
  wipe_staging(S, nullptr);
  (void)hipStreamSynchronize(nullptr);
  delete c->ed25519_sign;
  c->ed25519_sign = nullptr;
}

static int ensure_comb(cess_bls_ctx* c) {
  Ed25519SignState& S = sg_state(c);
  if (S.have_comb) return CESS_BLS_OK;
  hipStream_t s = c->stream;
  if (S.comb.ensure(ed25519::kCombWords * 4) | S.comb_status.ensure(ed25519::kCombRows)) return CESS_BLS_E_OOM;
  LAUNCH(ST_ED25519_COMB, s, k_ed25519_comb, dim3(1), dim3(64), 0, s, S.comb.as<uint32_t>(),
         S.comb_status.as<uint8_t>());
  HIPCHK(hipGetLastError());
  uint8_t st[ed25519::kCombRows];
  HIPCHK(hipMemcpyAsync(st, S.comb_status.p, sizeof st, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (uint8_t v : st)
    if (v != ed25519::KEY_LOADED) return CESS_BLS_E_HIP;
  S.have_comb = true;
  return CESS_BLS_OK;
}

// k seeds (host bytes, offsets already checked) into table T on the context's stream
static int signers_run(cess_bls_ctx* c, SignerTable& T, size_t k, const uint8_t* seeds,
                       const std::vector<uint64_t>& offs, uint64_t first, uint64_t bytes, const uint8_t* expected,
                       uint8_t* pubs_out, std::vector<uint8_t>& status) {
  Ed25519SignState& S = sg_state(c);
  hipStream_t s = c->stream;
  const size_t rows = std::max<size_t>(k, 1);
  // the previous table is cleared before its buffers can be replaced, and the
  // table is empty until its rows and statuses are written
  wipe_table(T, s);
  if (T.a.ensure(rows * 32) | T.prefix.ensure(rows * 32) | T.pub.ensure(rows * 32) | T.status.ensure(rows))
    return CESS_BLS_E_OOM;
  status.assign(k, 0);
  if (k == 0) return CESS_BLS_OK;
  // the digest kernel fetches whole dwords (4 bytes of slack) and writes whole waves of digests
  int r = upload_msgs(s, seeds, first, bytes, offs, S.seed_in, S.seed_offs, 4);
  if (r) return r;
  if (S.seed_dig.ensure(64 * (k / 64 + 1) * 64) | (expected ? S.expected.ensure(32 * k) : 0)) return CESS_BLS_E_OOM;
  if (expected) HIPCHK(hipMemcpyAsync(S.expected.p, expected, 32 * k, hipMemcpyHostToDevice, s));
  LAUNCH(ST_RSA_DIGEST, s, k_rsa_digest512, dim3((unsigned)(k / 64 + 1)), dim3(64), 0, s, (uint64_t)k,
         (const uint8_t*)S.seed_in.as<uint8_t>(), (const uint64_t*)S.seed_offs.as<uint64_t>(), S.seed_dig.as<uint8_t>(),
         0u, (uint64_t*)nullptr, (int)CESS_RSA_DIGEST_SHA512);
  LAUNCH(ST_ED25519_SIGNERS, s, k_ed25519_signers, dim3(grid_for(k)), dim3(kBlock), 0, s, (uint64_t)k,
         (const uint32_t*)S.comb.as<uint32_t>(), (const uint64_t*)S.seed_offs.as<uint64_t>(),
         (const uint8_t*)S.seed_dig.as<uint8_t>(), expected ? (const uint8_t*)S.expected.as<uint8_t>() : nullptr,
         T.a.as<uint32_t>(), T.prefix.as<uint32_t>(), T.pub.as<uint32_t>(), T.status.as<uint8_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(status.data(), T.status.p, k, hipMemcpyDeviceToHost, s));
  if (pubs_out) HIPCHK(hipMemcpyAsync(pubs_out, T.pub.p, 32 * k, hipMemcpyDeviceToHost, s));
  T.n = (uint32_t)k;
  return CESS_BLS_OK;
}

static int load_signers(cess_bls_ctx* c, SignerTable& T, size_t k, const uint8_t* seeds, const uint64_t* seed_offsets,
                        const uint8_t* expected, uint8_t* pubs_out, int* status_out) {
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  int r = order_begin(c, s);
  if (r) return r;
  std::vector<uint64_t> offs;
  uint64_t first = 0, bytes = 0;
  if (k && !rebase_offsets(seed_offsets, 0, k, seeds != nullptr, offs, &first, &bytes)) return CESS_BLS_E_INVALID_ARG;
  r = ensure_comb(c);
  if (r) return r;
  std::vector<uint8_t> st;
  r = signers_run(c, T, k, seeds, offs, first, bytes, expected, pubs_out, st);
  wipe_staging(sg_state(c), s);
  if (r) {
    wipe_table(T, s);
    return r;
  }
  HIPCHK(hipStreamSynchronize(s));
  if (status_out)
    for (size_t j = 0; j < k; j++)
      status_out[j] = st[j] == ed25519::SIGNER_LOADED    ? CESS_BLS_OK
                      : st[j] == ed25519::SIGNER_BAD_LEN ? CESS_BLS_E_BAD_KEY
                                                         : CESS_ED25519_E_INCONSISTENT;
  return call_end(c, s);
}

// device-resident records against table T, enqueued on s; msg_bytes = d_moffs[n] - d_moffs[0]
static int sign_run(cess_bls_ctx* c, SignerTable& T, hipStream_t s, uint64_t n, const uint32_t* d_idx,
                    const uint8_t* d_msgs, const uint64_t* d_moffs, uint64_t msg_bytes, uint8_t* d_sigs,
                    uint8_t* d_codes) {
  Ed25519SignState& S = sg_state(c);
  if (!S.have_comb) return CESS_BLS_E_INVALID_ARG;   // (every caller has built it)
  // the digest kernel fetches whole dwords (rsa_digest.hpp): 4 bytes of slack;
  // it writes whole waves of 64-byte digests
  if (T.a.ensure(32) | T.prefix.ensure(32) | T.pub.ensure(32) | T.status.ensure(1) |
      S.pack.ensure(64 * n + msg_bytes + 4) | S.pack_offs.ensure((n + 1) * 8) |
      S.digests.ensure(64 * (n / 64 + 1) * 64) | S.nonces.ensure(32 * n))
    return CESS_BLS_E_OOM;
  const uint8_t* status = T.status.as<uint8_t>();
  for (int pass = 0; pass < 2; pass++) {
    // pass 0: prefix || msg -> r, R; pass 1: R || A || msg -> k, S
    LAUNCH(ST_ED25519_SIGN_PACK, s, k_ed25519_sign_pack, dim3((unsigned)(n / kBlock + 1)), dim3(kBlock), 0, s, n, d_idx,
           T.n, status, (const uint8_t*)(pass ? T.pub.as<uint8_t>() : T.prefix.as<uint8_t>()),
           (const uint8_t*)(pass ? d_sigs : nullptr), d_msgs, d_moffs, S.pack.as<uint8_t>(), S.pack_offs.as<uint64_t>());
    LAUNCH(ST_RSA_DIGEST, s, k_rsa_digest512, dim3((unsigned)(n / 64 + 1)), dim3(64), 0, s, n,
           (const uint8_t*)S.pack.as<uint8_t>(), (const uint64_t*)S.pack_offs.as<uint64_t>(), S.digests.as<uint8_t>(), 0u,
           (uint64_t*)nullptr, (int)CESS_RSA_DIGEST_SHA512);
    if (pass == 0)
      LAUNCH(ST_ED25519_SIGN_R, s, k_ed25519_sign_r, dim3(grid_for(n)), dim3(kBlock), 0, s, n, d_idx, T.n, status,
             (const uint32_t*)S.comb.as<uint32_t>(), (const uint8_t*)S.digests.as<uint8_t>(), S.nonces.as<uint32_t>(),
             d_sigs);
    else
      LAUNCH(ST_ED25519_SIGN_S, s, k_ed25519_sign_s, dim3(grid_for(n)), dim3(kBlock), 0, s, n, d_idx, T.n, status,
             (const uint32_t*)T.a.as<uint32_t>(), (const uint8_t*)S.digests.as<uint8_t>(),
             (const uint32_t*)S.nonces.as<uint32_t>(), d_sigs, d_codes);
  }
  HIPCHK(hipGetLastError());
  return CESS_BLS_OK;
}

static int sign_host(cess_bls_ctx* c, SignerTable& T, size_t n, const uint32_t* signer_idx, const uint8_t* msgs,
                     const uint64_t* moffs, uint8_t* sigs_out, uint8_t* codes_out) {
  if (n == 0) return CESS_BLS_OK;
  if (!signer_idx || !moffs || !sigs_out || n >= (1ull << 31)) return CESS_BLS_E_INVALID_ARG;
  Ed25519SignState& S = sg_state(c);
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  int r = order_begin(c, s);
  if (r) return r;
  std::vector<uint64_t> mo;   // live until the synchronisation below
  uint64_t m0, mb;
  if (!rebase_offsets(moffs, 0, n, msgs != nullptr, mo, &m0, &mb)) return CESS_BLS_E_INVALID_ARG;
  r = ensure_comb(c);
  if (r) return r;
  if (S.in_idx.ensure(n * 4) | S.out_sigs.ensure(64 * n) | S.out_codes.ensure(n)) return CESS_BLS_E_OOM;
  r = upload_msgs(s, msgs, m0, mb, mo, S.in_msgs, S.in_moffs);
  if (r) return r;
  HIPCHK(hipMemcpyAsync(S.in_idx.p, signer_idx, n * 4, hipMemcpyHostToDevice, s));
  r = sign_run(c, T, s, n, S.in_idx.as<uint32_t>(), S.in_msgs.as<uint8_t>(), S.in_moffs.as<uint64_t>(), mb,
               S.out_sigs.as<uint8_t>(), S.out_codes.as<uint8_t>());
  wipe_staging(S, s);
  if (r) return r;
  HIPCHK(hipMemcpyAsync(sigs_out, S.out_sigs.p, 64 * n, hipMemcpyDeviceToHost, s));
  if (codes_out) HIPCHK(hipMemcpyAsync(codes_out, S.out_codes.p, n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return call_end(c, s);
}

extern "C" int cess_ed25519_signers_load(cess_bls_ctx* c, size_t k, const uint8_t* seeds, const uint64_t* seed_offsets,
                                         const uint8_t* expected_pubs, uint8_t* pubs_out, int* status_out) {
  ENTRY(c);
  if ((k && !seed_offsets) || k > 0xffffffffull) return CESS_BLS_E_INVALID_ARG;
  if (c->subs.empty())
    return load_signers(c, sg_state(c).user, k, seeds, seed_offsets, expected_pubs, pubs_out, status_out);
  for (size_t d = 0; d < c->subs.size(); d++) {
    int r = load_signers(c->subs[d], sg_state(c->subs[d]).user, k, seeds, seed_offsets, expected_pubs,
                         d == 0 ? pubs_out : nullptr, d == 0 ? status_out : nullptr);
    if (r) return r;
  }
  return CESS_BLS_OK;
}

int cess_ed25519_sign_one(cess_bls_ctx* s, size_t n, const uint32_t* signer_idx, const uint8_t* msgs,
                          const uint64_t* moffs, uint8_t* sigs_out, uint8_t* codes_out) {
  return sign_host(s, sg_state(s).user, n, signer_idx, msgs, moffs, sigs_out, codes_out);
}

extern "C" int cess_ed25519_sign_batch(cess_bls_ctx* c, size_t n, const uint32_t* signer_idx, const uint8_t* msgs,
                                       const uint64_t* msg_offsets, uint8_t* sigs_out, uint8_t* codes_out) {
  ENTRY(c);
  if (!c->subs.empty()) return cess_multi_ed25519_sign(c, n, signer_idx, msgs, msg_offsets, sigs_out, codes_out);
  return sign_host(c, sg_state(c).user, n, signer_idx, msgs, msg_offsets, sigs_out, codes_out);
}

extern "C" int cess_ed25519_sign_batch_device(cess_bls_ctx* c, size_t n, const uint32_t* d_signer_idx,
                                              const uint8_t* d_msgs, const uint64_t* d_msg_offsets, uint8_t* d_sigs_out,
                                              uint8_t* d_codes, void* stream) {
  ENTRY(c);
  if (!c->subs.empty() || (n && (!d_signer_idx || !d_msg_offsets || !d_sigs_out)) || n >= (1ull << 31))
    return CESS_BLS_E_INVALID_ARG;
  if (n == 0) return CESS_BLS_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  int r = order_begin(c, s);
  if (r) return r;
  // (the comb table is built on the context's stream and waited for, once per context)
  r = ensure_comb(c);
  if (r) return r;
  // the staging buffer's size: the two ends of the message range
  uint64_t ends[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&ends[0], d_msg_offsets, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&ends[1], d_msg_offsets + n, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (ends[1] < ends[0]) return CESS_BLS_E_INVALID_ARG;
  Ed25519SignState& S = sg_state(c);
  r = sign_run(c, S.user, s, n, d_signer_idx, d_msgs, d_msg_offsets, ends[1] - ends[0], d_sigs_out, d_codes);
  wipe_staging(S, s);
  if (r) return r;
  return call_end(c, s);
}

extern "C" int cess_ed25519_sign(cess_bls_ctx* c, const uint8_t* seed, size_t seed_len, const uint8_t* msg,
                                 size_t msg_len, uint8_t* sig_out64, uint8_t* pub_out32) {
  ENTRY(c);
  if (!sig_out64 || (!seed && seed_len) || (!msg && msg_len)) return CESS_BLS_E_INVALID_ARG;
  cess_bls_ctx* d = c->subs.empty() ? c : c->subs[0];
  static const uint8_t zero = 0;
  const uint64_t so[2] = {0, seed_len};
  int st = CESS_BLS_OK;
  SignerTable& T = sg_state(d).single;
  uint8_t pub[32];
  int r = load_signers(d, T, 1, seed ? seed : &zero, so, nullptr, pub, &st);
  if (!r && !st) {
    const uint32_t idx = 0;
    const uint64_t mo[2] = {0, msg_len};
    uint8_t code = 0xff;
    r = sign_host(d, T, 1, &idx, msg ? msg : &zero, mo, sig_out64, &code);
    if (!r && code != CESS_ED25519_SIGN_OK) r = CESS_BLS_E_HIP;
  }
  // the one-signer table does not outlive the call
  (void)hipSetDevice(d->device);
  wipe_table(T, d->stream);
  if (r) return r;
  if (st) return st;
  if (pub_out32) memcpy(pub_out32, pub, 32);
  return CESS_BLS_OK;
}
