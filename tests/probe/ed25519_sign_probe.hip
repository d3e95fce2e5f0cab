// Test-only probe of the Ed25519 signer's primitives
// (cess_amd/csrc/ed25519_sign.hpp: clamp, sc_reduce256, sc_muladd, the comb
// table and ge_scalarmult_base): one small kernel per operation, one lane per
// row, so that tests/test_gpu_ed25519_sign_primitives.py can compare every
// primitive with integer arithmetic on the tables of
// tests/golden/ed25519_sign_edges.json.  The header is included unchanged;
// nothing here is linked into libcess_bls.so (cess_amd/csrc/Makefile builds
// libcess_ed25519_sign_probe.so with the flags of k_ed25519_sign).
//
// Lane i reads n_in words at in[i * n_in ..] and writes n_out words at
// out[i * n_out ..].  The kernels take the production block and launch bounds:
// CESS_LB (256 threads), and one block of 64 threads with
// __launch_bounds__(64, 1) for the comb build, as k_ed25519_comb.
// ge_scalarmult_base reads a comb table that the probe builds first, on the
// device, with its own comb kernel.
//
// The lane functions are plain CESS_HD code: the host build
// (tests/hostemu/ed25519_sign_emu.cpp, -DCESS_HOSTEMU) includes this file and
// runs the same functions in a loop over the lanes.
#if !defined(CESS_HOSTEMU)
#include <hip/hip_runtime.h>
#endif

#include "../../cess_amd/csrc/ed25519_sign.hpp"
#include "../../cess_amd/csrc/kernels.hpp"

// entry, words in, words out
#define EDSP_OPS(X)        \
  X(clamp, 8, 8)           \
  X(sc_reduce256, 8, 8)    \
  X(sc_muladd, 24, 8)      \
  X(ge_scalarmult_base, 8, 8)

namespace edsp {
using namespace ed25519;

template <int N>
CESS_HD void ldw(const uint32_t* p, uint32_t (&w)[N]) {
#pragma unroll
  for (int i = 0; i < N; i++) w[i] = p[i];
}
template <int N>
CESS_HD void stw(uint32_t* p, const uint32_t (&w)[N]) {
#pragma unroll
  for (int i = 0; i < N; i++) p[i] = w[i];
}

// every lane function: (the lane's words in, its words out, the comb table)
CESS_HD void l_clamp(const uint32_t* in, uint32_t* out, const uint32_t*) {
  uint32_t a[8];
  ldw(in, a);
  clamp(a);
  stw(out, a);
}
CESS_HD void l_sc_reduce256(const uint32_t* in, uint32_t* out, const uint32_t*) {
  uint32_t a[8], r[8];
  ldw(in, a);
  sc_reduce256(a, r);
  stw(out, r);
}
// in: k, a, r
CESS_HD void l_sc_muladd(const uint32_t* in, uint32_t* out, const uint32_t*) {
  uint32_t k[8], a[8], r[8], s[8];
  ldw(in, k), ldw(in + 8, a), ldw(in + 16, r);
  sc_muladd(k, a, r, s);
  stw(out, s);
}
// in: a scalar below L; out: the 32 bytes of [s]B as 8 words
CESS_HD void l_ge_scalarmult_base(const uint32_t* in, uint32_t* out, const uint32_t* comb) {
  uint32_t s[8], e[8];
  ldw(in, s);
  ge_scalarmult_base(comb, s, e);
  stw(out, e);
}

// what the lanes' bounds forbid: a lane count outside [1, 2^16], a missing
// array, a scalar of ge_scalarmult_base that is not below L (its digits would
// not be those of the scalar)
inline bool args_ok(bool scalars, uint32_t n, const uint32_t* in, const uint32_t* out) {
  if (n == 0 || n > (1u << 16) || !in || !out) return false;
  if (scalars)
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t* s = in + (uint64_t)i * 8;
      int q = 7;
      while (q > 0 && s[q] == kL[q]) q--;
      if (s[q] >= kL[q]) return false;
    }
  return true;
}

}  // namespace edsp

#if !defined(CESS_HOSTEMU)
struct EdspArgs {
  uint32_t n;   // lanes
  const uint32_t* in;
  uint32_t* out;
  const uint32_t* comb;
};

#define X(name, NI, NO)                                                          \
  __global__ CESS_LB void k_edsp_##name(EdspArgs g) {                            \
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;                    \
    if (i >= g.n) return;                                                        \
    edsp::l_##name(g.in + (uint64_t)i * NI, g.out + (uint64_t)i * NO, g.comb);   \
  }
EDSP_OPS(X)
#undef X

__global__ __launch_bounds__(64, 1) void k_edsp_comb(uint32_t* comb, uint8_t* status) {
  const int i = threadIdx.x;
  if (blockIdx.x != 0 || i >= ed25519::kCombRows) return;
  status[i] = ed25519::comb_row(i, comb + (uint64_t)ed25519::kTableWords * i);
}

// hipMalloc, copy in, (comb build,) launch, hipDeviceSynchronize, copy out,
// free; returns the HIP status (or hipErrorInvalidValue for arguments the
// lanes' bounds forbid)
template <typename Kern>
static int edsp_run(Kern kern, uint32_t n_in, uint32_t n_out, bool with_comb, uint32_t n, const uint32_t* in,
                    uint32_t* out) {
  if (!edsp::args_ok(with_comb, n, in, out)) return (int)hipErrorInvalidValue;
  const size_t in_b = (size_t)n * n_in * sizeof(uint32_t), out_b = (size_t)n * n_out * sizeof(uint32_t);
  uint32_t *d_in = nullptr, *d_out = nullptr, *d_comb = nullptr;
  uint8_t* d_st = nullptr;
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  if (ok(hipMalloc(&d_in, in_b)) && ok(hipMalloc(&d_out, out_b)) &&
      (!with_comb || (ok(hipMalloc(&d_comb, ed25519::kCombWords * 4)) && ok(hipMalloc(&d_st, ed25519::kCombRows)))) &&
      ok(hipMemcpy(d_in, in, in_b, hipMemcpyHostToDevice)) && ok(hipMemcpy(d_out, out, out_b, hipMemcpyHostToDevice))) {
    if (with_comb) hipLaunchKernelGGL(k_edsp_comb, dim3(1), dim3(64), 0, 0, d_comb, d_st);
    const EdspArgs g{n, d_in, d_out, d_comb};
    hipLaunchKernelGGL(kern, dim3((n + 255) / 256), dim3(256), 0, 0, g);
    if (ok(hipGetLastError()) && ok(hipDeviceSynchronize())) ok(hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost));
  }
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  (void)hipFree(d_comb);
  (void)hipFree(d_st);
  return (int)e;
}

extern "C" {
int edsp_clamp(uint32_t n, const uint32_t* in, uint32_t* out) { return edsp_run(k_edsp_clamp, 8, 8, false, n, in, out); }
int edsp_sc_reduce256(uint32_t n, const uint32_t* in, uint32_t* out) {
  return edsp_run(k_edsp_sc_reduce256, 8, 8, false, n, in, out);
}
int edsp_sc_muladd(uint32_t n, const uint32_t* in, uint32_t* out) {
  return edsp_run(k_edsp_sc_muladd, 24, 8, false, n, in, out);
}
int edsp_ge_scalarmult_base(uint32_t n, const uint32_t* in, uint32_t* out) {
  return edsp_run(k_edsp_ge_scalarmult_base, 8, 8, true, n, in, out);
}
// the comb table (64 x 240 words) and the 64 row statuses
int edsp_comb(uint32_t* comb, uint8_t* status) {
  if (!comb || !status) return (int)hipErrorInvalidValue;
  uint32_t* d_comb = nullptr;
  uint8_t* d_st = nullptr;
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  if (ok(hipMalloc(&d_comb, ed25519::kCombWords * 4)) && ok(hipMalloc(&d_st, ed25519::kCombRows))) {
    hipLaunchKernelGGL(k_edsp_comb, dim3(1), dim3(64), 0, 0, d_comb, d_st);
    if (ok(hipGetLastError()) && ok(hipDeviceSynchronize()) &&
        ok(hipMemcpy(comb, d_comb, ed25519::kCombWords * 4, hipMemcpyDeviceToHost)))
      ok(hipMemcpy(status, d_st, ed25519::kCombRows, hipMemcpyDeviceToHost));
  }
  (void)hipFree(d_comb);
  (void)hipFree(d_st);
  return (int)e;
}
const char* ed25519_sign_probe_error(int status) { return hipGetErrorString((hipError_t)status); }
}
#endif
