// Host side of the ECDSA P-256 batch verifier (include/cess_ecdsa.h): the key
// table (k_ecdsa_keys), and per batch the signature split and the hash input
// (k_ecdsa_pack), the digests (k_rsa_digest, or k_rsa_digest512 for SHA-384, as
// the hashed RSA mode launches them, prefix = 0) and the verification
// (k_ecdsa_verify).  Staging, launches and the call end are host.hpp's, exactly
// as in host_ed25519.cpp.
#include "host.hpp"

#include "p256.hpp"

using namespace cess_host;

__global__ void k_ecdsa_keys(uint64_t, const uint8_t*, const uint64_t*, uint32_t*, uint8_t*);
__global__ void k_ecdsa_pack(uint64_t, uint32_t, const uint8_t*, const uint64_t*, const uint8_t*, const uint64_t*,
                             uint8_t*, uint64_t*, uint32_t*);
__global__ void k_ecdsa_verify(uint64_t, const uint32_t*, uint32_t, const uint8_t*, const uint32_t*, const uint32_t*,
                               const uint32_t*, const uint8_t*, uint32_t, uint8_t*);

// per-context ECDSA key tables: the caller's and a one-key table for cess_ecdsa_verify
struct EcTable {
  DevBuf tab, status;
  uint32_t n = 0;
};
struct EcdsaState {
  EcTable user, single, base;   // base: the multiples of G, built once per context
  bool have_base = false;
  DevBuf key_in, key_offs, in_idx, in_sigs, in_soffs, in_msgs, in_moffs, out_codes;
  DevBuf pack, pack_offs, digests, rec;
};

static EcdsaState& ec_state(cess_bls_ctx* c) {
  if (!c->ecdsa) c->ecdsa = new EcdsaState();
  return *c->ecdsa;
}
void cess_ecdsa_state_free(cess_bls_ctx* c) {
  delete c->ecdsa;
  c->ecdsa = nullptr;
}

static bool alg_ok(int alg) { return alg >= CESS_ECDSA_ALG_P256_SHA256_FIXED && alg <= CESS_ECDSA_ALG_P256_SHA384_ASN1; }

// k keys (host bytes, offsets already checked) into table T on the context's stream; status bytes back
static int table_run(cess_bls_ctx* c, EcTable& T, size_t k, const uint8_t* keys, const std::vector<uint64_t>& offs,
                     uint64_t first, uint64_t bytes, std::vector<uint8_t>& status) {
  EcdsaState& S = ec_state(c);
  hipStream_t s = c->stream;
  const size_t rows = std::max<size_t>(k, 1);
  // the table is empty until its rows and statuses are written: a load that
  // fails part-way leaves no table, never one with undefined statuses
  T.n = 0;
  if (T.tab.ensure(rows * p256::kTableWords * 4) | T.status.ensure(rows)) return CESS_BLS_E_OOM;
  status.assign(k, 0);
  if (k == 0) return CESS_BLS_OK;
  int r = upload_msgs(s, keys, first, bytes, offs, S.key_in, S.key_offs);
  if (r) return r;
  LAUNCH(ST_ECDSA_KEYS, s, k_ecdsa_keys, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, s, (uint64_t)k,
         (const uint8_t*)S.key_in.as<uint8_t>(), (const uint64_t*)S.key_offs.as<uint64_t>(), T.tab.as<uint32_t>(),
         T.status.as<uint8_t>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(status.data(), T.status.p, k, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  T.n = (uint32_t)k;
  return CESS_BLS_OK;
}

static int ensure_base(cess_bls_ctx* c) {
  EcdsaState& S = ec_state(c);
  if (S.have_base) return CESS_BLS_OK;
  const std::vector<uint64_t> offs = {0, 65};
  std::vector<uint8_t> st;
  int r = table_run(c, S.base, 1, p256::kGEnc, offs, 0, 65, st);
  if (r) return r;
  if (st[0] != p256::KEY_LOADED) return CESS_BLS_E_HIP;
  S.have_base = true;
  return CESS_BLS_OK;
}

static int load_table(cess_bls_ctx* c, EcTable& T, size_t k, const uint8_t* keys, const uint64_t* key_offsets,
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
    for (size_t j = 0; j < k; j++) status_out[j] = st[j] == p256::KEY_LOADED ? CESS_BLS_OK : CESS_BLS_E_BAD_KEY;
  return call_end(c, c->stream);
}

// device-resident records against table T, enqueued on s; msg_bytes = d_moffs[n] - d_moffs[0]
static int ec_run(cess_bls_ctx* c, EcTable& T, hipStream_t s, int alg, uint64_t n, const uint32_t* d_idx,
                  const uint8_t* d_sigs, const uint64_t* d_soffs, const uint8_t* d_msgs, const uint64_t* d_moffs,
                  uint64_t msg_bytes, uint8_t* d_codes) {
  EcdsaState& S = ec_state(c);
  if (!S.have_base) return CESS_BLS_E_INVALID_ARG;   // (every caller has loaded a table)
  const bool sha384 = alg == CESS_ECDSA_ALG_P256_SHA384_ASN1;
  const uint32_t stride = sha384 ? 48u : 32u;
  // the digest kernels fetch whole dwords (rsa_digest.hpp): 4 bytes of slack;
  // they write whole waves of digests
  if (T.tab.ensure(p256::kTableWords * 4) | T.status.ensure(1) | S.pack.ensure(msg_bytes + 4) |
      S.pack_offs.ensure((n + 1) * 8) | S.digests.ensure(64 * (n / 64 + 1) * 64) |
      S.rec.ensure(n * p256::kRecWords * 4))
    return CESS_BLS_E_OOM;
  LAUNCH(ST_ECDSA_PACK, s, k_ecdsa_pack, dim3((unsigned)(n / kBlock + 1)), dim3(kBlock), 0, s, n, (uint32_t)alg, d_sigs,
         d_soffs, d_msgs, d_moffs, S.pack.as<uint8_t>(), S.pack_offs.as<uint64_t>(), S.rec.as<uint32_t>());
  if (sha384)
    LAUNCH(ST_RSA_DIGEST, s, k_rsa_digest512, dim3((unsigned)(n / 64 + 1)), dim3(64), 0, s, n,
           (const uint8_t*)S.pack.as<uint8_t>(), (const uint64_t*)S.pack_offs.as<uint64_t>(), S.digests.as<uint8_t>(),
           0u, (uint64_t*)nullptr, (int)CESS_RSA_DIGEST_SHA384);
  else
    LAUNCH(ST_RSA_DIGEST, s, k_rsa_digest, dim3((unsigned)(n / 64 + 1)), dim3(64), 0, s, n,
           (const uint8_t*)S.pack.as<uint8_t>(), (const uint64_t*)S.pack_offs.as<uint64_t>(), S.digests.as<uint8_t>(),
           0u, (uint64_t*)nullptr);
  LAUNCH(ST_ECDSA_VERIFY, s, k_ecdsa_verify, dim3(grid_for(n)), dim3(kBlock), 0, s, n, d_idx, T.n,
         (const uint8_t*)T.status.as<uint8_t>(), (const uint32_t*)T.tab.as<uint32_t>(),
         (const uint32_t*)S.base.tab.as<uint32_t>(), (const uint32_t*)S.rec.as<uint32_t>(),
         (const uint8_t*)S.digests.as<uint8_t>(), stride, d_codes);
  HIPCHK(hipGetLastError());
  return CESS_BLS_OK;
}

static int ec_host(cess_bls_ctx* c, EcTable& T, int alg, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                   const uint64_t* soffs, const uint8_t* msgs, const uint64_t* moffs, uint8_t* codes_out,
                   uint64_t* bitmap_out) {
  if (n == 0) return CESS_BLS_OK;
  if (!key_idx || !soffs || !moffs || n >= (1ull << 31)) return CESS_BLS_E_INVALID_ARG;
  EcdsaState& S = ec_state(c);
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
  r = ec_run(c, T, s, alg, n, S.in_idx.as<uint32_t>(), S.in_sigs.as<uint8_t>(), S.in_soffs.as<uint64_t>(),
             S.in_msgs.as<uint8_t>(), S.in_moffs.as<uint64_t>(), mb, S.out_codes.as<uint8_t>());
  if (r) return r;
  std::vector<uint8_t> codes(n);
  HIPCHK(hipMemcpyAsync(codes.data(), S.out_codes.p, n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (codes_out) memcpy(codes_out, codes.data(), n);
  if (bitmap_out) bitmap_from_codes(codes.data(), n, bitmap_out);
  return call_end(c, s);
}

extern "C" int cess_ecdsa_keys_load(cess_bls_ctx* c, size_t k, const uint8_t* keys, const uint64_t* key_offsets,
                                    int* key_status_out) {
  ENTRY(c);
  if ((k && !key_offsets) || k > 0xffffffffull) return CESS_BLS_E_INVALID_ARG;
  if (c->subs.empty()) return load_table(c, ec_state(c).user, k, keys, key_offsets, key_status_out);
  for (size_t d = 0; d < c->subs.size(); d++) {
    int r = load_table(c->subs[d], ec_state(c->subs[d]).user, k, keys, key_offsets, d == 0 ? key_status_out : nullptr);
    if (r) return r;
  }
  return CESS_BLS_OK;
}

int cess_ecdsa_one(cess_bls_ctx* s, int alg, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                   const uint64_t* soffs, const uint8_t* msgs, const uint64_t* moffs, uint8_t* codes_out,
                   uint64_t* bitmap_out) {
  return ec_host(s, ec_state(s).user, alg, n, key_idx, sigs, soffs, msgs, moffs, codes_out, bitmap_out);
}

extern "C" int cess_ecdsa_verify_batch(cess_bls_ctx* c, int alg, size_t n, const uint32_t* key_idx, const uint8_t* sigs,
                                       const uint64_t* sig_offsets, const uint8_t* msgs, const uint64_t* msg_offsets,
                                       uint8_t* codes_out, uint64_t* bitmap_out) {
  if (!alg_ok(alg)) return CESS_BLS_E_INVALID_ARG;
  ENTRY(c);
  if (!c->subs.empty())
    return cess_multi_ecdsa(c, alg, n, key_idx, sigs, sig_offsets, msgs, msg_offsets, codes_out, bitmap_out);
  return ec_host(c, ec_state(c).user, alg, n, key_idx, sigs, sig_offsets, msgs, msg_offsets, codes_out, bitmap_out);
}

extern "C" int cess_ecdsa_verify_batch_device(cess_bls_ctx* c, int alg, size_t n, const uint32_t* d_key_idx,
                                              const uint8_t* d_sigs, const uint64_t* d_sig_offsets,
                                              const uint8_t* d_msgs, const uint64_t* d_msg_offsets, uint8_t* d_codes,
                                              void* stream) {
  if (!alg_ok(alg)) return CESS_BLS_E_INVALID_ARG;
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
  r = ec_run(c, ec_state(c).user, s, alg, n, d_key_idx, d_sigs, d_sig_offsets, d_msgs, d_msg_offsets,
             ends[1] - ends[0], d_codes);
  if (r) return r;
  return call_end(c, s);
}

extern "C" int cess_ecdsa_verify(cess_bls_ctx* c, int alg, const uint8_t* key, size_t key_len, const uint8_t* msg,
                                 size_t msg_len, const uint8_t* sig, size_t sig_len, int* ok_out) {
  if (!alg_ok(alg)) return CESS_BLS_E_INVALID_ARG;
  ENTRY(c);
  if (!ok_out || (!key && key_len) || (!msg && msg_len) || (!sig && sig_len)) return CESS_BLS_E_INVALID_ARG;
  *ok_out = 0;
  cess_bls_ctx* d = c->subs.empty() ? c : c->subs[0];
  static const uint8_t zero = 0;
  const uint64_t ko[2] = {0, key_len};
  int st = CESS_BLS_OK;
  EcTable& T = ec_state(d).single;
  int r = load_table(d, T, 1, key ? key : &zero, ko, &st);
  if (r) return r;
  if (st) return st;
  const uint32_t idx = 0;
  const uint64_t so[2] = {0, sig_len}, mo[2] = {0, msg_len};
  uint8_t code = 0xff;
  r = ec_host(d, T, alg, 1, &idx, sig ? sig : &zero, so, msg ? msg : &zero, mo, &code, nullptr);
  if (r) return r;
  *ok_out = code == CESS_ECDSA_OK;
  return CESS_BLS_OK;
}
