// Host side of the Ed25519 batch verifier (include/cess_ed25519.h): the key
// table (k_ed25519_keys), and per batch the hash input (k_ed25519_pack), the
// digests (k_rsa_digest512 as the hashed RSA mode launches it, prefix = 0,
// SHA-512) and the verification (k_ed25519_verify).  Staging, launches and the
// call end are host.hpp's; the host-buffer entry stages like host_rsa.cpp's.
#include "host.hpp"

#include "ed25519.hpp"

using namespace cess_host;

__global__ void k_ed25519_keys(uint64_t, const uint8_t*, const uint64_t*, uint32_t*, uint8_t*, uint8_t*);
__global__ void k_ed25519_pack(uint64_t, const uint32_t*, uint32_t, const uint8_t*, const uint8_t*, const uint64_t*,
                               const uint8_t*, const uint64_t*, uint8_t*, uint64_t*);
__global__ void k_ed25519_verify(uint64_t, const uint32_t*, uint32_t, const uint8_t*, const uint32_t*, const uint32_t*,
                                 const uint8_t*, const uint64_t*, const uint8_t*, uint8_t*);

// per-context Ed25519 key tables: the caller's and a one-key table for cess_ed25519_verify
struct EdTable {
  DevBuf tab, status, raw;
  uint32_t n = 0;
};
struct Ed25519State {
  EdTable user, single, base;   // base: the multiples of B, built once per context
  bool have_base = false;
  DevBuf key_in, key_offs, in_idx, in_sigs, in_soffs, in_msgs, in_moffs, out_codes;
  DevBuf pack, pack_offs, digests;
};

static Ed25519State& ed_state(cess_bls_ctx* c) {
  if (!c->ed25519) c->ed25519 = new Ed25519State();
  return *c->ed25519;
}
void cess_ed25519_state_free(cess_bls_ctx* c) {
  delete c->ed25519;
  c->ed25519 = nullptr;
}

// k keys (host bytes, offsets already checked) into table T on the context's stream; status bytes back
static int table_run(cess_bls_ctx* c, EdTable& T, size_t k, const uint8_t* keys, const std::vector<uint64_t>& offs,
                     uint64_t first, uint64_t bytes, std::vector<uint8_t>& status) {
  Ed25519State& S = ed_state(c);
  hipStream_t s = c->stream;
  const size_t rows = std::max<size_t>(k, 1);
  // the table is empty until its rows and statuses are written: a load that
  // fails part-way leaves no table, never one with undefined statuses
  T.n = 0;
  if (T.tab.ensure(rows * ed25519::kTableWords * 4) | T.status.ensure(rows) | T.raw.ensure(rows * 32))
    return CESS_BLS_E_OOM;
  status.assign(k, 0);
  if (k == 0) return CESS_BLS_OK;
  int r = upload_msgs(s, keys, first, bytes, offs, S.key_in, S.key_offs);
  if (r) return r;
  LAUNCH(ST_ED25519_KEYS, s, k_ed25519_keys, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, s, (uint64_t)k,
         (const uint8_t*)S.key_in.as<uint8_t>(), (const uint64_t*)S.key_offs.as<uint64_t>(), T.tab.as<uint32_t>(),
         T.status.as<uint8_t>(), T.raw.as<uint8_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(status.data(), T.status.p, k, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  T.n = (uint32_t)k;
  return CESS_BLS_OK;
}

static int ensure_base(cess_bls_ctx* c) {
  Ed25519State& S = ed_state(c);
  if (S.have_base) return CESS_BLS_OK;
  const std::vector<uint64_t> offs = {0, 32};
  std::vector<uint8_t> st;
  int r = table_run(c, S.base, 1, ed25519::kNegBaseEnc, offs, 0, 32, st);
  if (r) return r;
  if (st[0] != ed25519::KEY_LOADED) return CESS_BLS_E_HIP;
  S.have_base = true;
  return CESS_BLS_OK;
}

static int load_table(cess_bls_ctx* c, EdTable& T, size_t k, const uint8_t* keys, const uint64_t* key_offsets,
                      int* status_out) {
  HIPCHK(hipSetDevice(c->device));
  int r = order_begin(c, c->stream);
  if (r) return r;
  std::vector<uint64_t> offs;
  uint64_t first = 0, bytes = 0;
  if (k && !rebase_offsets(key_offsets, 0, k, keys != nullptr, offs, &first, &bytes)) return CESS_BLS_E_INVALID_ARG;
  r = ensure_base(c);
  if (r) return r;
  std::vector<uint8_t> st;
  r = table_run(c, T, k, keys, offs, first, bytes, st);
  if (r) return r;
  if (status_out)
    for (size_t j = 0; j < k; j++) status_out[j] = st[j] == ed25519::KEY_LOADED ? CESS_BLS_OK : CESS_BLS_E_BAD_KEY;
  return call_end(c, c->stream);
}

// device-resident records against table T, enqueued on s; msg_bytes = d_moffs[n] - d_moffs[0]
static int ed_run(cess_bls_ctx* c, EdTable& T, hipStream_t s, uint64_t n, const uint32_t* d_idx, const uint8_t* d_sigs,
                  const uint64_t* d_soffs, const uint8_t* d_msgs, const uint64_t* d_moffs, uint64_t msg_bytes,
                  uint8_t* d_codes) {
  Ed25519State& S = ed_state(c);
  if (!S.have_base) return CESS_BLS_E_INVALID_ARG;   // (every caller has loaded a table)
  // the digest kernel fetches whole dwords (rsa_digest.hpp): 4 bytes of slack;
  // it writes whole waves of 64-byte digests
  if (T.tab.ensure(ed25519::kTableWords * 4) | T.status.ensure(1) | T.raw.ensure(32) |
      S.pack.ensure(64 * n + msg_bytes + 4) | S.pack_offs.ensure((n + 1) * 8) | S.digests.ensure(64 * (n / 64 + 1) * 64))
    return CESS_BLS_E_OOM;
  LAUNCH(ST_ED25519_PACK, s, k_ed25519_pack, dim3((unsigned)(n / kBlock + 1)), dim3(kBlock), 0, s, n, d_idx, T.n,
         (const uint8_t*)T.raw.as<uint8_t>(), d_sigs, d_soffs, d_msgs, d_moffs, S.pack.as<uint8_t>(),
         S.pack_offs.as<uint64_t>());
  LAUNCH(ST_RSA_DIGEST, s, k_rsa_digest512, dim3((unsigned)(n / 64 + 1)), dim3(64), 0, s, n,
         (const uint8_t*)S.pack.as<uint8_t>(), (const uint64_t*)S.pack_offs.as<uint64_t>(), S.digests.as<uint8_t>(), 0u,
         (uint64_t*)nullptr, (int)CESS_RSA_DIGEST_SHA512);
  LAUNCH(ST_ED25519_VERIFY, s, k_ed25519_verify, dim3(grid_for(n)), dim3(kBlock), 0, s, n, d_idx, T.n,
         (const uint8_t*)T.status.as<uint8_t>(), (const uint32_t*)T.tab.as<uint32_t>(),
         (const uint32_t*)S.base.tab.as<uint32_t>(), d_sigs, d_soffs, (const uint8_t*)S.digests.as<uint8_t>(), d_codes);
  HIPCHK(hipGetLastError());
  return CESS_BLS_OK;
}

static int ed_host(cess_bls_ctx* c, EdTable& T, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                   const uint64_t* soffs, const uint8_t* msgs, const uint64_t* moffs, uint8_t* codes_out,
                   uint64_t* bitmap_out) {
  if (n == 0) return CESS_BLS_OK;
  if (!key_idx || !soffs || !moffs || n >= (1ull << 31)) return CESS_BLS_E_INVALID_ARG;
  Ed25519State& S = ed_state(c);
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  int r = order_begin(c, s);
  if (r) return r;
  std::vector<uint64_t> so, mo;   // live until the synchronisation below
  uint64_t s0, sb, m0, mb;
  if (!rebase_offsets(soffs, 0, n, sigs != nullptr, so, &s0, &sb) ||
      !rebase_offsets(moffs, 0, n, msgs != nullptr, mo, &m0, &mb))
    return CESS_BLS_E_INVALID_ARG;
  r = ensure_base(c);
  if (r) return r;
  if (S.in_idx.ensure(n * 4) | S.out_codes.ensure(n)) return CESS_BLS_E_OOM;
  r = upload_msgs(s, sigs, s0, sb, so, S.in_sigs, S.in_soffs);
  if (!r) r = upload_msgs(s, msgs, m0, mb, mo, S.in_msgs, S.in_moffs);
  if (r) return r;
  HIPCHK(hipMemcpyAsync(S.in_idx.p, key_idx, n * 4, hipMemcpyHostToDevice, s));
  r = ed_run(c, T, s, n, S.in_idx.as<uint32_t>(), S.in_sigs.as<uint8_t>(), S.in_soffs.as<uint64_t>(),
             S.in_msgs.as<uint8_t>(), S.in_moffs.as<uint64_t>(), mb, S.out_codes.as<uint8_t>());
  if (r) return r;
  std::vector<uint8_t> codes(n);
  HIPCHK(hipMemcpyAsync(codes.data(), S.out_codes.p, n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (codes_out) memcpy(codes_out, codes.data(), n);
  if (bitmap_out) bitmap_from_codes(codes.data(), n, bitmap_out);
  return call_end(c, s);
}

extern "C" int cess_ed25519_keys_load(cess_bls_ctx* c, size_t k, const uint8_t* keys, const uint64_t* key_offsets,
                                      int policy, int* key_status_out) {
  if (policy != CESS_ED25519_POLICY_RING) return CESS_BLS_E_INVALID_ARG;
  ENTRY(c);
  if ((k && !key_offsets) || k > 0xffffffffull) return CESS_BLS_E_INVALID_ARG;
  if (c->subs.empty()) return load_table(c, ed_state(c).user, k, keys, key_offsets, key_status_out);
  for (size_t d = 0; d < c->subs.size(); d++) {
    int r = load_table(c->subs[d], ed_state(c->subs[d]).user, k, keys, key_offsets, d == 0 ? key_status_out : nullptr);
    if (r) return r;
  }
  return CESS_BLS_OK;
}

int cess_ed25519_one(cess_bls_ctx* s, size_t n, const uint32_t* key_idx, const uint8_t* sigs, const uint64_t* soffs,
                     const uint8_t* msgs, const uint64_t* moffs, uint8_t* codes_out, uint64_t* bitmap_out) {
  return ed_host(s, ed_state(s).user, n, key_idx, sigs, soffs, msgs, moffs, codes_out, bitmap_out);
}

extern "C" int cess_ed25519_verify_batch(cess_bls_ctx* c, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                                         const uint64_t* sig_offsets, const uint8_t* msgs, const uint64_t* msg_offsets,
                                         uint8_t* codes_out, uint64_t* bitmap_out) {
  ENTRY(c);
  if (!c->subs.empty())
    return cess_multi_ed25519(c, n, key_idx, sigs, sig_offsets, msgs, msg_offsets, codes_out, bitmap_out);
  return ed_host(c, ed_state(c).user, n, key_idx, sigs, sig_offsets, msgs, msg_offsets, codes_out, bitmap_out);
}

extern "C" int cess_ed25519_verify_batch_device(cess_bls_ctx* c, size_t n, const uint32_t* d_key_idx,
                                                const uint8_t* d_sigs, const uint64_t* d_sig_offsets,
                                                const uint8_t* d_msgs, const uint64_t* d_msg_offsets, uint8_t* d_codes,
                                                void* stream) {
  ENTRY(c);
  if (!c->subs.empty() || (n && (!d_key_idx || !d_sig_offsets || !d_msg_offsets || !d_codes)) || n >= (1ull << 31))
    return CESS_BLS_E_INVALID_ARG;
  if (n == 0) return CESS_BLS_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  int r = order_begin(c, s);
  if (r) return r;
  // (the base table is built on the context's stream and waited for, once per context)
  r = ensure_base(c);
  if (r) return r;
  // the staging buffer's size: the two ends of the message range
  uint64_t ends[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&ends[0], d_msg_offsets, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&ends[1], d_msg_offsets + n, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (ends[1] < ends[0]) return CESS_BLS_E_INVALID_ARG;
  r = ed_run(c, ed_state(c).user, s, n, d_key_idx, d_sigs, d_sig_offsets, d_msgs, d_msg_offsets, ends[1] - ends[0],
             d_codes);
  if (r) return r;
  return call_end(c, s);
}

extern "C" int cess_ed25519_verify(cess_bls_ctx* c, const uint8_t* key, size_t key_len, const uint8_t* msg,
                                   size_t msg_len, const uint8_t* sig, size_t sig_len, int policy, int* ok_out) {
  if (policy != CESS_ED25519_POLICY_RING) return CESS_BLS_E_INVALID_ARG;
  ENTRY(c);
  if (!ok_out || (!key && key_len) || (!msg && msg_len) || (!sig && sig_len)) return CESS_BLS_E_INVALID_ARG;
  *ok_out = 0;
  cess_bls_ctx* d = c->subs.empty() ? c : c->subs[0];
  static const uint8_t zero = 0;
  const uint64_t ko[2] = {0, key_len};
  int st = CESS_BLS_OK;
  EdTable& T = ed_state(d).single;
  int r = load_table(d, T, 1, key ? key : &zero, ko, &st);
  if (r) return r;
  if (st) return st;
  const uint32_t idx = 0;
  const uint64_t so[2] = {0, sig_len}, mo[2] = {0, msg_len};
  uint8_t code = 0xff;
  r = ed_host(d, T, 1, &idx, sig ? sig : &zero, so, msg ? msg : &zero, mo, &code, nullptr);
  if (r) return r;
  *ok_out = code == CESS_ED25519_OK;
  return CESS_BLS_OK;
}
