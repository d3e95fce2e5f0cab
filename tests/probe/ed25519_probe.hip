// Test-only probe of the Ed25519 primitives (cess_amd/csrc/ed25519.hpp: the
// field, the scalars, the group formulas, the key table and the verify loop):
// one small kernel per operation, one lane per row, so that
// tests/test_gpu_ed25519_primitives.py can compare every primitive with integer
// arithmetic on the operand tables of tests/ed25519_probe_model.py.  The header
// is included unchanged; nothing here is linked into libcess_bls.so
// (cess_amd/csrc/Makefile builds libcess_ed25519_probe.so with the flags of
// k_ed25519_verify).
//
// Lane i reads n_in words at in[i * n_in ..] and writes n_out words at
// out[i * n_out ..]; the layouts are listed in tests/ed25519_probe_model.py.
// Lanes whose `active` byte is zero return at once and leave their results
// untouched.  The kernels take the production block and launch bounds: CESS_LB
// (256 threads), and 64 threads with __launch_bounds__(64, 1) for key_table, as
// k_ed25519_keys.  ge_pre_digit and verify_equation read their tables from
// device memory through ge_pre_load's uint2 path.
//
// The lane functions are plain CESS_HD code: the host build
// (tests/hostemu/ed25519_emu.cpp, -DCESS_HOSTEMU) includes this file and runs
// the same functions in a loop over the lanes.
#if !defined(CESS_HOSTEMU)
#include <hip/hip_runtime.h>
#endif

#include "../../cess_amd/csrc/ed25519.hpp"
#include "../../cess_amd/csrc/kernels.hpp"

// entry, words in, words out, leading table indices among the words in, threads per block
#define EDP_OPS(X)                \
  X(fe_mul, 20, 10, 0, 256)       \
  X(fe_sqr, 10, 10, 0, 256)       \
  X(fe_add, 20, 10, 0, 256)       \
  X(fe_sub, 20, 10, 0, 256)       \
  X(fe_neg, 10, 10, 0, 256)       \
  X(fe_carry, 10, 10, 0, 256)     \
  X(fe_neg_tight, 10, 10, 0, 256) \
  X(fe_from_words, 8, 10, 0, 256) \
  X(fe_to_words, 10, 10, 0, 256)  \
  X(fe_invert, 10, 10, 0, 256)    \
  X(fe_pow22523, 10, 10, 0, 256)  \
  X(sc_lt_L, 8, 1, 0, 256)        \
  X(sc_reduce512, 16, 8, 0, 256)  \
  X(sc_digits, 8, 64, 0, 256)     \
  X(ge_dbl, 30, 80, 0, 256)       \
  X(ge_madd, 70, 80, 0, 256)      \
  X(ge_decode, 8, 21, 0, 256)     \
  X(key_table, 9, 241, 0, 64)     \
  X(ge_pre_digit, 2, 30, 1, 256)  \
  X(verify_equation, 26, 1, 2, 256)

namespace edp {
using namespace ed25519;

CESS_HD fe ld(const uint32_t* p) {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = p[i];
  return r;
}
CESS_HD void st(uint32_t* p, const fe& a) {
#pragma unroll
  for (int i = 0; i < 10; i++) p[i] = a.v[i];
}
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
CESS_HD void l_fe_carry(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, fe_carry(ld(in))); }
CESS_HD void l_fe_neg_tight(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, fe_neg_tight(ld(in))); }
CESS_HD void l_fe_invert(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, fe_invert(ld(in))); }
CESS_HD void l_fe_pow22523(const uint32_t* in, uint32_t* out, const uint32_t*) { st(out, fe_pow22523(ld(in))); }
CESS_HD void l_fe_from_words(const uint32_t* in, uint32_t* out, const uint32_t*) {
  uint32_t w[8];
  ldw(in, w);
  st(out, fe_from_words(w));
}
CESS_HD void l_fe_to_words(const uint32_t* in, uint32_t* out, const uint32_t*) {
  const fe a = ld(in);
  uint32_t w[8];
  fe_to_words(a, w);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = w[i];
  out[8] = fe_is_zero(a) ? 1u : 0u;
  out[9] = fe_is_negative(a);
}
CESS_HD void l_sc_lt_L(const uint32_t* in, uint32_t* out, const uint32_t*) {
  uint32_t s[8];
  ldw(in, s);
  out[0] = sc_lt_L(s) ? 1u : 0u;
}
CESS_HD void l_sc_reduce512(const uint32_t* in, uint32_t* out, const uint32_t*) {
  uint32_t x[16], r[8];
  ldw(in, x);
  sc_reduce512(x, r);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = r[i];
}
// the 64 digits, most significant first, as the verify loop reads them, each plus 8
CESS_HD void l_sc_digits(const uint32_t* in, uint32_t* out, const uint32_t*) {
  uint32_t s[8], r[8];
  ldw(in, s);
  sc_recode(s, r);
#pragma unroll 1
  for (int i = 0; i < 64; i++) out[i] = (uint32_t)(sc_top_digit(r) + 8);
}
CESS_HD void st_factors(uint32_t* out, ge_p3& p, const fe& E, const fe& H, const fe& G, const fe& F) {
  st(out, E), st(out + 10, H), st(out + 20, G), st(out + 30, F);
  ge_finish(p, E, H, G, F, true);
  st(out + 40, p.X), st(out + 50, p.Y), st(out + 60, p.Z), st(out + 70, p.T);
}
CESS_HD void l_ge_dbl(const uint32_t* in, uint32_t* out, const uint32_t*) {
  ge_p3 p = {ld(in), ld(in + 10), ld(in + 20), fe_small(0)};
  fe E, H, G, F;
  ge_dbl(p, E, H, G, F);
  st_factors(out, p, E, H, G, F);
}
CESS_HD void l_ge_madd(const uint32_t* in, uint32_t* out, const uint32_t*) {
  ge_p3 p = {ld(in), ld(in + 10), ld(in + 20), ld(in + 30)};
  const ge_pre q = {ld(in + 40), ld(in + 50), ld(in + 60)};
  fe E, H, G, F;
  ge_madd(p, q, E, H, G, F);
  st_factors(out, p, E, H, G, F);
}
CESS_HD void l_ge_decode(const uint32_t* in, uint32_t* out, const uint32_t*) {
  uint32_t w[8];
  ldw(in, w);
  fe x, y;
  out[0] = ge_decode(w, x, y) ? 1u : 0u;
  st(out + 1, x), st(out + 11, y);
}
// in: the length, then the key's bytes as 8 little-endian words; out: the status, then the table
CESS_HD void l_key_table(const uint32_t* in, uint32_t* out, const uint32_t*) {
  out[0] = key_table(reinterpret_cast<const uint8_t*>(in + 1), in[0], out + 1);
}
// in: the table's index (checked by the caller against the table count), the digit plus 8
CESS_HD void l_ge_pre_digit(const uint32_t* in, uint32_t* out, const uint32_t* tabs) {
  const ge_pre q = ge_pre_digit(tabs + (uint64_t)kTableWords * in[0], (int)in[1] - 8);
  st(out, q.ypx), st(out + 10, q.ymx), st(out + 20, q.xy2d);
}
// in: the indices of the key's table and of the base point's, S, h, R
CESS_HD void l_verify_equation(const uint32_t* in, uint32_t* out, const uint32_t* tabs) {
  uint32_t S[8], h[8], R[8];
  ldw(in + 2, S), ldw(in + 10, h), ldw(in + 18, R);
  out[0] = verify_equation(tabs + (uint64_t)kTableWords * in[0], tabs + (uint64_t)kTableWords * in[1], S, h, R) ? 1u : 0u;
}

// what the lanes' bounds forbid: a lane count outside [1, 2^16], a missing
// array, a table index outside the tables, a digit outside [-8, 8]
inline bool args_ok(uint32_t n_in, uint32_t n_idx, uint32_t n, const uint8_t* active, const uint32_t* in, const uint32_t* out,
                    const uint32_t* tabs, uint32_t n_tabs) {
  if (n == 0 || n > (1u << 16) || !active || !in || !out || n_tabs > (1u << 12)) return false;
  if (n_idx && (!tabs || n_tabs == 0)) return false;
  for (uint32_t i = 0; i < n; i++) {
    for (uint32_t j = 0; j < n_idx; j++)
      if (in[(uint64_t)i * n_in + j] >= n_tabs) return false;
    if (n_idx == 1 && in[(uint64_t)i * n_in + 1] > 16) return false;
  }
  return true;
}

}  // namespace edp

#if !defined(CESS_HOSTEMU)
struct EdpArgs {
  uint32_t n;              // lanes
  const uint8_t* active;   // per lane
  const uint32_t* in;
  uint32_t* out;
  const uint32_t* tabs;
};

#define EDP_LB_256 CESS_LB
#define EDP_LB_64 __launch_bounds__(64, 1)
#define X(name, NI, NO, NIDX, T)                                               \
  __global__ EDP_LB_##T void k_edp_##name(EdpArgs g) {                         \
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;                  \
    if (i >= g.n || !g.active[i]) return;                                      \
    edp::l_##name(g.in + (uint64_t)i * NI, g.out + (uint64_t)i * NO, g.tabs);  \
  }
EDP_OPS(X)
#undef X

// hipMalloc, copy in, launch, hipDeviceSynchronize, copy out, free; returns the
// HIP status (or hipErrorInvalidValue for arguments the lanes' bounds forbid).
// `out` arrives pre-filled by the caller (poison) and is copied in, so the
// results of inactive lanes come back as they went in.
template <typename Kern>
static int edp_run(Kern kern, uint32_t n_in, uint32_t n_out, uint32_t n_idx, uint32_t threads, uint32_t n,
                   const uint8_t* active, const uint32_t* in, uint32_t* out, const uint32_t* tabs, uint32_t n_tabs) {
  if (!edp::args_ok(n_in, n_idx, n, active, in, out, tabs, n_tabs)) return (int)hipErrorInvalidValue;
  const size_t in_b = (size_t)n * n_in * sizeof(uint32_t), out_b = (size_t)n * n_out * sizeof(uint32_t);
  const size_t tab_b = n_idx ? (size_t)n_tabs * ed25519::kTableWords * sizeof(uint32_t) : 0;
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
    const EdpArgs g{n, d_act, d_in, d_out, d_tabs};
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
#define X(name, NI, NO, NIDX, T)                                                                                  \
  int edp_##name(uint32_t n, const uint8_t* active, const uint32_t* in, uint32_t* out, const uint32_t* tabs,      \
                 uint32_t n_tabs) {                                                                                \
    return edp_run(k_edp_##name, NI, NO, NIDX, T, n, active, in, out, tabs, n_tabs);                               \
  }
EDP_OPS(X)
#undef X

// "name:words in:words out:table indices:threads,..." of every entry point
const char* ed25519_probe_ops() {
  return ""
#define X(name, NI, NO, NIDX, T) #name ":" #NI ":" #NO ":" #NIDX ":" #T ","
      EDP_OPS(X)
#undef X
      ;
}
const char* ed25519_probe_error(int status) { return hipGetErrorString((hipError_t)status); }
}
#endif
