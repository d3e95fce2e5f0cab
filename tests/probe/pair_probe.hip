// Test-only probe of the lane-pair primitives (bls/pair.hpp, bls/pair_fe.hpp):
// one small kernel per operation, in the production launch shape (blocks of
// CESS_PAIR_THREADS, two blocks per CU, pair i on threads 2i and 2i + 1, the
// Fp12 accumulator in the LDS image G[18][CESS_PAIR_THREADS], HBM slots as
// GlobPair views that start at the wave's first signature), so that
// tests/test_gpu_pair_primitives.py can compare every primitive with integer
// arithmetic mod p.  The headers are included unchanged; nothing here is linked
// into libcess_bls.so (cess_amd/csrc/Makefile builds libcess_pair_probe.so).
//
// Operands and results are raw Montgomery limbs exactly as the kernels hold
// them: value v of pair i is 2 x 12 words at in[((i * n_in + v) * 2 + h) * 12],
// h the component (= the lane of the pair that holds it); results likewise in
// `out`.  A predicate is returned as a word per lane (limb 0 of that lane's
// component of result 0, the other limbs zero).  Pairs whose `active` byte is
// zero return at once, both lanes together, and leave their results untouched.
#include <hip/hip_runtime.h>
#include <string.h>
#include "soa.hpp"
#include "bls/pair_fe.hpp"

using namespace bls;

// name, operands, results (Fp2 values per pair)
#define PP_OPS(X)                \
  X(xchg, 1, 1)                  \
  X(partner_signed, 1, 1)        \
  X(mul_nr, 1, 1)                \
  X(mul_nr_nr, 1, 1)             \
  X(add_xi_nr, 2, 1)             \
  X(conj, 1, 1)                  \
  X(fph_one, 0, 1)               \
  X(is_zero, 1, 1)               \
  X(eq, 2, 1)                    \
  X(pmul_scaled1, 2, 1)          \
  X(pmul_scaled2, 2, 1)          \
  X(pmul_scaled3, 2, 1)          \
  X(psqr, 1, 1)                  \
  X(pdot2, 4, 1)                 \
  X(pmul_fp, 2, 1)               \
  X(pinv, 1, 1)                  \
  X(pmul_p, 2, 1)                \
  X(pdot2_p, 4, 1)               \
  X(pmul6, 6, 3)                 \
  X(pmul_by_1, 4, 3)             \
  X(pmul_by_01_one, 4, 3)        \
  X(psqr12, 6, 6)                \
  X(pmul014, 9, 6)               \
  X(pmul014_one, 8, 6)           \
  X(pmul12, 12, 6)               \
  X(pinv12, 6, 6)                \
  X(pfrob12, 6, 6)               \
  X(pfp4_square, 2, 2)           \
  X(pcyc_square_run, 6, 6)       \
  X(pkcyc_run_ps, 4, 4)          \
  X(pcyc_z1_frac, 4, 2)          \
  X(pcyc_z1_den, 2, 1)           \
  X(pcyc_z0, 5, 1)               \
  X(pcyc_chain, 6, 18)           \
  X(pis_one12, 6, 1)             \
  X(pis_conj12, 12, 1)           \
  X(glob_roundtrip, 6, 12)

enum Op : int {
#define X(name, ni, no) OP_##name,
  PP_OPS(X)
#undef X
      OP_COUNT
};

constexpr int kSlots = 4;   // HBM slots of 36 rows x stride uint4 each

struct Args {
  uint32_t n;              // pairs
  const uint8_t* active;   // per pair
  const uint32_t* in;
  uint32_t* out;
  uint32_t n_in, n_out;
  int arg;                 // n of the runs, k of pfrob12, the store of pis_one12
  uint4* slots;
  uint64_t stride;
};

template <int OP>
__global__ __launch_bounds__(CESS_PAIR_THREADS, 2) void k_probe(Args a) {
  // as k_final2: signature of the pair; both lanes take every branch together
  const uint32_t i = blockIdx.x * (blockDim.x >> 1) + (threadIdx.x >> 1);
  const uint32_t h = threadIdx.x & 1u;
  if (i >= a.n || !a.active[i]) return;

  auto in_c = [&](int v, uint32_t comp) {
    const uint32_t* p = a.in + (((uint64_t)i * a.n_in + v) * 2 + comp) * 12;
    fp r;
#pragma unroll
    for (int w = 0; w < 12; w++) r.v[w] = p[w];
    return r;
  };
  auto in = [&](int v) { return fph{in_c(v, h)}; };
  auto in_full = [&](int v) { return fp2{in_c(v, 0), in_c(v, 1)}; };
  auto out_c = [&](int v, uint32_t comp, const fp& x) {
    uint32_t* p = a.out + (((uint64_t)i * a.n_out + v) * 2 + comp) * 12;
#pragma unroll
    for (int w = 0; w < 12; w++) p[w] = x.v[w];
  };
  auto out = [&](int v, const fph& x) { out_c(v, h, x.v); };
  auto out_full = [&](int v, const fp2& x) {
    out_c(v, 0, x.c0);
    out_c(v, 1, x.c1);
  };
  auto out_pred = [&](bool b) {
    fp r = fp_zero();
    r.v[0] = b ? 1u : 0u;
    out_c(0, h, r);
  };
  auto out6 = [&](int v, const fp6h& x) {
    out(v, x.c0);
    out(v + 1, x.c1);
    out(v + 2, x.c2);
  };
  // slot views start at the wave's first signature (uniform), as k_final2
  const uint32_t s0 = blockIdx.x * (blockDim.x >> 1) + (wave_first_thread() >> 1);
  auto slot = [&](int s) { return GlobPair{a.slots + (uint64_t)s * 36 * a.stride + s0, a.stride}; };

  constexpr bool lds = OP == OP_psqr12 || OP == OP_pmul014 || OP == OP_pmul014_one || OP == OP_pmul12 ||
                       OP == OP_pinv12 || OP == OP_pfrob12 || OP == OP_pcyc_square_run || OP == OP_pis_one12 ||
                       OP == OP_pis_conj12;
  if constexpr (lds) {
    __shared__ uint4 G[18][CESS_PAIR_THREADS];
    const LdsPair f{G, wave_first_thread()};
#pragma unroll 1
    for (int k = 0; k < 6; k++) f.st(k, in(k));
    CESS_MEMBAR();
    bool store = true;
    if constexpr (OP == OP_psqr12) psqr12(f);
    if constexpr (OP == OP_pmul014) pmul014(f, in(6), in(7), in(8));
    if constexpr (OP == OP_pmul014_one) pmul014_one(f, in(6), in(7));
    if constexpr (OP == OP_pmul12 || OP == OP_pis_conj12) {
      const GlobPair g = slot(0);
#pragma unroll 1
      for (int k = 0; k < 6; k++) g.st(k, in(6 + k));
      CESS_MEMBAR();
      if constexpr (OP == OP_pmul12) {
        pmul12(f, g);
      } else {
        out_pred(pis_conj12(f, g));
        store = false;
      }
    }
    if constexpr (OP == OP_pinv12) pinv12(f);
    if constexpr (OP == OP_pfrob12) pfrob12(f, a.arg);
    if constexpr (OP == OP_pcyc_square_run) pcyc_square_run(f, a.arg);
    if constexpr (OP == OP_pis_one12) {
      if (a.arg) {   // uniform: the HBM store (k_final2 asks slot(SL_F)) or the LDS accumulator
        const GlobPair g = slot(0);
        pcopy12(g, f);
        CESS_MEMBAR();
        out_pred(pis_one12(g));
      } else {
        out_pred(pis_one12(f));
      }
      store = false;
    }
    CESS_MEMBAR();
    if (store) {
#pragma unroll 1
      for (int k = 0; k < 6; k++) out(k, f.ld(k));
    }
  }

  if constexpr (OP == OP_xchg) out(0, fph{xchg(in(0).v)});
  if constexpr (OP == OP_partner_signed) out(0, fph{partner_signed(in(0).v)});
  if constexpr (OP == OP_mul_nr) out(0, mul_nr(in(0)));
  if constexpr (OP == OP_mul_nr_nr) out(0, mul_nr_nr(in(0)));
  if constexpr (OP == OP_add_xi_nr) out(0, add_xi_nr(in(0), in(1)));
  if constexpr (OP == OP_conj) out(0, conj(in(0)));
  if constexpr (OP == OP_fph_one) out(0, fph_one());
  if constexpr (OP == OP_is_zero) out_pred(is_zero(in(0)));
  if constexpr (OP == OP_eq) out_pred(eq(in(0), in(1)));
  if constexpr (OP == OP_pmul_scaled1) out(0, pmul_scaled<1>(in(0), in(1)));
  if constexpr (OP == OP_pmul_scaled2) out(0, pmul_scaled<2>(in(0), in(1)));
  if constexpr (OP == OP_pmul_scaled3) out(0, pmul_scaled<3>(in(0), in(1)));
  if constexpr (OP == OP_psqr) out(0, psqr(in(0)));
  if constexpr (OP == OP_pdot2) out(0, pdot2(in(0), in(1), in(2), in(3)));
  if constexpr (OP == OP_pmul_fp) out(0, pmul_fp(in(0), in_c(1, 0)));   // s: component 0 of operand 1, in both lanes
  if constexpr (OP == OP_pinv) out(0, pinv(in(0)));
  if constexpr (OP == OP_pmul_p) out(0, pmul_p(prep_x(in(0)), prep_y(in(1))));
  if constexpr (OP == OP_pdot2_p) out(0, pdot2_p(prep_x(in(0)), prep_y(in(1)), prep_x(in(2)), prep_y(in(3))));
  if constexpr (OP == OP_pmul6) out6(0, pmul6({in(0), in(1), in(2)}, {in(3), in(4), in(5)}));
  if constexpr (OP == OP_pmul_by_1) out6(0, pmul_by_1({in(0), in(1), in(2)}, in(3)));
  if constexpr (OP == OP_pmul_by_01_one) out6(0, pmul_by_01_one({in(0), in(1), in(2)}, in(3)));
  if constexpr (OP == OP_pfp4_square) {
    fph c0, c1;
    pfp4_square(c0, c1, in(0), in(1));
    out(0, c0);
    out(1, c1);
  }
  if constexpr (OP == OP_pkcyc_run_ps) {
    // operands z2, z3, z4, z5; lane 0 holds (u, w) = (z4, z5), lane 1 (z3, z2)
    const int vu = h ? 1 : 2, vw = h ? 0 : 3;
    fp2 u = in_full(vu), w = in_full(vw);
    pkcyc_run_ps(u, w, a.arg);
    out_full(vu, u);
    out_full(vw, w);
  }
  if constexpr (OP == OP_pcyc_z1_frac) {   // z2, z3, z4, z5 -> num, den
    fph num, den;
    pcyc_z1_frac(in(0), in(1), in(2), in(3), num, den);
    out(0, num);
    out(1, den);
  }
  if constexpr (OP == OP_pcyc_z1_den) out(0, pcyc_z1_den(in(0), in(1)));
  if constexpr (OP == OP_pcyc_z0) out(0, pcyc_z0(in(0), in(1), in(2), in(3), in(4)));   // z1 .. z5
  if constexpr (OP == OP_pcyc_chain) {
    const GlobPair base = slot(0);
#pragma unroll 1
    for (int k = 0; k < 6; k++) base.st(k, in(k));
    CESS_MEMBAR();
    pcyc_chain(base, [&](int j) { return slot(1 + j); });
    CESS_MEMBAR();
#pragma unroll 1
    for (int j = 0; j < 3; j++) {
      const GlobPair x = slot(1 + j);
#pragma unroll 1
      for (int k = 0; k < 6; k++) out(6 * j + k, x.ld(k));
    }
  }
  if constexpr (OP == OP_glob_roundtrip) {
    // st / ld by component through slot 0, then ld_full / st_full of whole
    // coefficients (a different one per lane, as pcyc_chain) into slot 1,
    // read back by component
    const GlobPair g0 = slot(0), g1 = slot(1);
#pragma unroll 1
    for (int k = 0; k < 6; k++) g0.st(k, in(k));
    CESS_MEMBAR();
#pragma unroll 1
    for (int k = 0; k < 6; k++) out(k, g0.ld(k));
#pragma unroll 1
    for (int j = 0; j < 3; j++) {
      const int k = h ? 2 + j : (j == 0 ? 1 : j == 1 ? 5 : 0);   // lane 0: 1, 5, 0; lane 1: 2, 3, 4
      g1.st_full(k, g0.ld_full(k));
    }
    CESS_MEMBAR();
#pragma unroll 1
    for (int k = 0; k < 6; k++) out(6 + k, g1.ld(k));
  }
}

// hipMalloc, copy in, launch, hipDeviceSynchronize, copy out, free; returns the
// HIP status (or hipErrorInvalidValue for arguments the kernels' bounds forbid).
// `out` arrives pre-filled by the caller (poison) and is copied in, so the
// results of inactive pairs come back as they went in.  raw_slots (optional):
// the kSlots x 36 x stride uint4 slot image after the run.
template <int OP>
static int run(uint32_t n_in, uint32_t n_out, uint32_t n, const uint8_t* active, const uint32_t* in, uint32_t* out,
               int arg, uint64_t stride, uint32_t* raw_slots) {
  if (n == 0 || n > (1u << 16) || stride < n || stride > (1u << 20) || !active || !out || (n_in && !in) || arg < 0 ||
      arg > 64)
    return (int)hipErrorInvalidValue;
  const size_t in_b = (size_t)n * (n_in ? n_in : 1) * 24 * sizeof(uint32_t), out_b = (size_t)n * n_out * 24 * sizeof(uint32_t);
  const size_t slot_b = (size_t)kSlots * 36 * stride * sizeof(uint4);
  uint8_t* d_act = nullptr;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  uint4* d_slots = nullptr;
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  if (ok(hipMalloc(&d_act, n)) && ok(hipMalloc(&d_in, in_b)) && ok(hipMalloc(&d_out, out_b)) &&
      ok(hipMalloc(&d_slots, slot_b)) && ok(hipMemcpy(d_act, active, n, hipMemcpyHostToDevice)) &&
      ok(n_in ? hipMemcpy(d_in, in, in_b, hipMemcpyHostToDevice) : hipSuccess) &&
      ok(hipMemcpy(d_out, out, out_b, hipMemcpyHostToDevice)) && ok(hipMemset(d_slots, 0xA5, slot_b))) {
    const Args a{n, d_act, d_in, d_out, n_in, n_out, arg, d_slots, stride};
    const uint32_t per = CESS_PAIR_THREADS / 2;
    hipLaunchKernelGGL(k_probe<OP>, dim3((n + per - 1) / per), dim3(CESS_PAIR_THREADS), 0, 0, a);
    if (ok(hipGetLastError()) && ok(hipDeviceSynchronize()) && ok(hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost)) &&
        raw_slots)
      ok(hipMemcpy(raw_slots, d_slots, slot_b, hipMemcpyDeviceToHost));
  }
  (void)hipFree(d_act);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  (void)hipFree(d_slots);
  return (int)e;
}

extern "C" {
#define X(name, ni, no)                                                                                              \
  int pp_##name(uint32_t n, const uint8_t* active, const uint32_t* in, uint32_t* out, int arg, uint64_t stride,    \
                uint32_t* raw_slots) {                                                                               \
    return run<OP_##name>(ni, no, n, active, in, out, arg, stride, raw_slots);                                       \
  }
PP_OPS(X)
#undef X

// "name:operands:results,..." of every entry point above
const char* pair_probe_ops() {
  return ""
#define X(name, ni, no) #name ":" #ni ":" #no ","
      PP_OPS(X)
#undef X
      ;
}
int pair_probe_threads() { return CESS_PAIR_THREADS; }
int pair_probe_slots() { return kSlots; }
const char* pair_probe_error(int status) { return hipGetErrorString((hipError_t)status); }
}
