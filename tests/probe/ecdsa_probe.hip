// Test-only probe of the ECDSA P-256 primitives (cess_amd/csrc/p256.hpp: the
// field, the scalars, the recoding, the group formulas, the key table, the
// signature parser and the verify loop): one small kernel per operation, one
// lane per row, so that tests/test_gpu_ecdsa_primitives.py can compare every
// primitive with integer arithmetic.  The header is included unchanged; nothing
// here is linked into libcess_bls.so (cess_amd/csrc/Makefile builds
// libcess_ecdsa_probe.so with the flags of k_ecdsa_verify).
//
// Lane i reads n_in words at in[i * n_in ..] and writes n_out words at
// out[i * n_out ..]; the layouts are given at the lane functions.  Lanes whose
// `active` byte is zero return at once and leave their results untouched.  The
// kernels take the production block and launch bounds: CESS_LB (256 threads),
// and 64 threads with __launch_bounds__(64, 1) for key_table, as k_ecdsa_keys.
//
// The lane functions are plain CESS_HD code: the host build
// (tests/hostemu/ecdsa_emu.cpp, -DCESS_HOSTEMU) includes this file and runs the
// same functions in a loop over the lanes.
#if !defined(CESS_HOSTEMU)
#include <hip/hip_runtime.h>
#endif

#include "../../cess_amd/csrc/kernels.hpp"
#include "../../cess_amd/csrc/p256.hpp"

// entry, words in, words out, leading table indices among the words in, threads
// per block, the position of a byte length among the words in plus one (0:
// none) and the bytes that follow it at most
#define ECP_OPS(X)                        \
  X(fe_mul, 20, 10, 0, 256, 0, 0)         \
  X(fe_sqr, 10, 10, 0, 256, 0, 0)         \
  X(fe_add, 20, 10, 0, 256, 0, 0)         \
  X(fe_sub, 20, 10, 0, 256, 0, 0)         \
  X(fe_neg, 10, 10, 0, 256, 0, 0)         \
  X(fe_mulk, 11, 10, 0, 256, 0, 0)        \
  X(fe_canon, 10, 11, 0, 256, 0, 0)       \
  X(fe_invert, 10, 10, 0, 256, 0, 0)      \
  X(sc_mul, 20, 10, 0, 256, 0, 0)         \
  X(sc_sqr, 10, 10, 0, 256, 0, 0)         \
  X(sc_invert, 10, 10, 0, 256, 0, 0)      \
  X(sc_canon, 10, 10, 0, 256, 0, 0)       \
  X(sc_digits, 8, 65, 0, 256, 0, 0)       \
  X(digest_scalar, 8, 8, 0, 256, 0, 0)    \
  X(pt_dbl, 30, 30, 0, 256, 0, 0)         \
  X(pt_madd, 50, 30, 0, 256, 0, 0)        \
  X(key_table, 18, 241, 0, 64, 1, 68)     \
  X(parse_sig, 82, 17, 0, 256, 2, 320)    \
  X(double_mul, 18, 30, 2, 256, 0, 0)     \
  X(verify_scalars, 26, 1, 2, 256, 0, 0)

namespace ecp {
using namespace p256;

CESS_HD fe ld(const uint32_t* p) { return fe_load(p); }
CESS_HD void st(uint32_t* p, const fe& a) { fe_store(p, a); }
template <int N>
CESS_HD void ldw(const uint32_t* p, uint32_t (&w)[N]) {
#pragma unroll
  for (int i = 0; i < N; i++) w[i] = p[i];
}

// every lane function: (the lane's words in, its words out, the tables)
CESS_HD void l_fe_mul(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, fe_mul(ld(in), ld(in + 10))); }
CESS_HD void l_fe_sqr(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, fe_sqr(ld(in))); }
CESS_HD void l_fe_add(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, fe_add(ld(in), ld(in + 10))); }
CESS_HD void l_fe_sub(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, fe_sub(ld(in), ld(in + 10))); }
CESS_HD void l_fe_neg(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, fe_neg(ld(in))); }
// in: a, then k (1..8, checked by the caller)
CESS_HD void l_fe_mulk(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, fe_mulk(ld(in), in[10])); }
// out: the canonical digits, then fe_is_zero
CESS_HD void l_fe_canon(const uint32_t* in, uint32_t* out, const uint32_t*) {
  st(out, canon_mod<kQ>(ld(in)));
  out[10] = fe_is_zero(ld(in)) ? 1u : 0u;
}
CESS_HD void l_fe_invert(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, fe_invert(ld(in))); }
CESS_HD void l_sc_mul(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, sc_mul(ld(in), ld(in + 10))); }
CESS_HD void l_sc_sqr(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, sc_sqr(ld(in))); }
CESS_HD void l_sc_invert(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, sc_invert(ld(in))); }
CESS_HD void l_sc_canon(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, canon_mod<kN>(ld(in))); }
// the top digit (0 or 1), then the 64 digits, most significant first, as the ladder reads them, each plus 8
CESS_HD void l_sc_digits(const uint32_t* in, uint32_t* out, const uint32_t*) {
  uint32_t s[8], t[8];
  ldw(in, s);
  out[0] = sc_recode(s, t);
#pragma unroll 1
  for (int i = 0; i < 64; i++) out[1 + i] = (uint32_t)(sc_top_digit(t) + 8);
}
// in: 32 digest bytes as they lie in memory
CESS_HD void l_digest_scalar(const uint32_t* in, uint32_t* out, const uint32_t*) {
  uint32_t e[8];
  digest_scalar(reinterpret_cast<const uint8_t*>(in), e);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = e[i];
}
CESS_HD void l_pt_dbl(const uint32_t* in, uint32_t* out, const uint32_t*) {
  const jac r = pt_dbl({ld(in), ld(in + 10), ld(in + 20)});
  st(out, r.X), st(out + 10, r.Y), st(out + 20, r.Z);
}
CESS_HD void l_pt_madd(const uint32_t* in, uint32_t* out, const uint32_t*) {
  const jac r = pt_madd({ld(in), ld(in + 10), ld(in + 20)}, ld(in + 30), ld(in + 40));
  st(out, r.X), st(out + 10, r.Y), st(out + 20, r.Z);
}
// in: the length, then the key's bytes; out: the status, then the table
CESS_HD void l_key_table(const uint32_t* in, uint32_t* out, const uint32_t*) {
  out[0] = key_table(reinterpret_cast<const uint8_t*>(in + 1), in[0], out + 1);
}
// in: the algorithm, the length, then the signature's bytes; out: r, s, the code
CESS_HD void l_parse_sig(const uint32_t* in, uint32_t* out, const uint32_t*) {
  uint32_t r[8], s[8];
  out[16] = parse_sig(in[0], reinterpret_cast<const uint8_t*>(in + 2), in[1], r, s);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = r[i], out[8 + i] = s[i];
}
// in: the indices of Q's table and of G's, u1, u2; out: u1 G + u2 Q (X, Y, Z)
CESS_HD void l_double_mul(const uint32_t* in, uint32_t* out, const uint32_t* tabs) {
  uint32_t u1[8], u2[8];
  ldw(in + 2, u1), ldw(in + 10, u2);
  const jac r = double_mul(tabs + (uint64_t)kTableWords * in[0], tabs + (uint64_t)kTableWords * in[1], u1, u2);
  st(out, r.X), st(out + 10, r.Y), st(out + 20, r.Z);
}
// in: the indices of the key's table and of G's, e, r, s
CESS_HD void l_verify_scalars(const uint32_t* in, uint32_t* out, const uint32_t* tabs) {
  uint32_t e[8], r[8], s[8];
  ldw(in + 2, e), ldw(in + 10, r), ldw(in + 18, s);
  out[0] = verify_scalars(tabs + (uint64_t)kTableWords * in[0], tabs + (uint64_t)kTableWords * in[1], e, r, s) ? 1u : 0u;
}

// what the lanes' bounds forbid: a lane count outside [1, 2^16], a missing
// array, a table index outside the tables, a byte length past the lane's words
inline bool args_ok(uint32_t n_in, uint32_t n_idx, uint32_t len_at, uint32_t len_max, uint32_t n, const uint8_t* active,
                    const uint32_t* in, const uint32_t* out, const uint32_t* tabs, uint32_t n_tabs) {
  if (n == 0 || n > (1u << 16) || !active || !in || !out || n_tabs > (1u << 12)) return false;
  if (n_idx && (!tabs || n_tabs == 0)) return false;
  for (uint32_t i = 0; i < n; i++) {
    for (uint32_t j = 0; j < n_idx; j++)
      if (in[(uint64_t)i * n_in + j] >= n_tabs) return false;
    if (len_at && in[(uint64_t)i * n_in + len_at - 1] > len_max) return false;
    if (n_in == 11 && (in[(uint64_t)i * n_in + 10] == 0 || in[(uint64_t)i * n_in + 10] > 8)) return false;   // fe_mulk's k
  }
  return true;
}

}  // namespace ecp

#if !defined(CESS_HOSTEMU)
struct EcpArgs {
  uint32_t n;              // lanes
  const uint8_t* active;   // per lane
  const uint32_t* in;
  uint32_t* out;
  const uint32_t* tabs;
};

#define ECP_LB_256 CESS_LB
#define ECP_LB_64 __launch_bounds__(64, 1)
#define X(name, NI, NO, NIDX, T, LA, LM)                                       \
  __global__ ECP_LB_##T void k_ecp_##name(EcpArgs g) {                         \
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;                  \
    if (i >= g.n || !g.active[i]) return;                                      \
    ecp::l_##name(g.in + (uint64_t)i * NI, g.out + (uint64_t)i * NO, g.tabs);  \
  }
ECP_OPS(X)
#undef X

// hipMalloc, copy in, launch, hipDeviceSynchronize, copy out, free; returns the
// HIP status (or hipErrorInvalidValue for arguments the lanes' bounds forbid).
// `out` arrives pre-filled by the caller (poison) and is copied in, so the
// results of inactive lanes come back as they went in.
template <typename Kern>
static int ecp_run(Kern kern, uint32_t n_in, uint32_t n_out, uint32_t n_idx, uint32_t threads, uint32_t len_at,
                   uint32_t len_max, uint32_t n, const uint8_t* active, const uint32_t* in, uint32_t* out,
                   const uint32_t* tabs, uint32_t n_tabs) {
  if (!ecp::args_ok(n_in, n_idx, len_at, len_max, n, active, in, out, tabs, n_tabs)) return (int)hipErrorInvalidValue;
  const size_t in_b = (size_t)n * n_in * sizeof(uint32_t), out_b = (size_t)n * n_out * sizeof(uint32_t);
  const size_t tab_b = n_idx ? (size_t)n_tabs * p256::kTableWords * sizeof(uint32_t) : 0;
  uint8_t* d_act = nullptr;
  uint32_t *d_in = nullptr, *d_out = nullptr, *d_tabs = nullptr;
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  if (ok(hipMalloc(&d_act, n)) && ok(hipMalloc(&d_in, in_b)) && ok(hipMalloc(&d_out, out_b)) &&
      (!tab_b || ok(hipMalloc(&d_tabs, tab_b))) && ok(hipMemcpy(d_act, active, n, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_in, in, in_b, hipMemcpyHostToDevice)) && ok(hipMemcpy(d_out, out, out_b, hipMemcpyHostToDevice)) &&
      (!tab_b || ok(hipMemcpy(d_tabs, tabs, tab_b, hipMemcpyHostToDevice)))) {
    const EcpArgs g{n, d_act, d_in, d_out, d_tabs};
    hipLaunchKernelGGL(kern, dim3((n + threads - 1) / threads), dim3(threads), 0, 0, g);
    if (ok(hipGetLastError()) && ok(hipDeviceSynchronize())) ok(hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost));
  }
  (void)hipFree(d_act);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  (void)hipFree(d_tabs);
  return (int)e;
}

extern "C" {
// tabs: n_tabs tables of 240 words (may be null for an entry that reads none)
#define X(name, NI, NO, NIDX, T, LA, LM)                                                                          \
  int ecp_##name(uint32_t n, const uint8_t* active, const uint32_t* in, uint32_t* out, const uint32_t* tabs,      \
                 uint32_t n_tabs) {                                                                                \
    return ecp_run(k_ecp_##name, NI, NO, NIDX, T, LA, LM, n, active, in, out, tabs, n_tabs);                       \
  }
ECP_OPS(X)
#undef X

// "name:words in:words out:table indices:threads,..." of every entry point
const char* ecdsa_probe_ops() {
  return ""
#define X(name, NI, NO, NIDX, T, LA, LM) #name ":" #NI ":" #NO ":" #NIDX ":" #T ","
      ECP_OPS(X)
#undef X
      ;
}
const char* ecdsa_probe_error(int status) { return hipGetErrorString((hipError_t)status); }
}
#endif
