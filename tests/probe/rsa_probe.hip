// Test-only probe of the RSA Montgomery primitives (k_rsa.hpp: mont<L, SQR>,
// canon, to_words; rsa_mont.hpp: mont_rt): one small kernel per operation, in
// blocks of 256 threads, one lane per row, so that
// tests/test_gpu_rsa_primitives.py can compare every primitive with integer
// arithmetic on the operand tables of tests/rsa_probe_model.py.  The headers
// are included unchanged; nothing here is linked into libcess_bls.so
// (cess_amd/csrc/Makefile builds libcess_rsa_probe.so).
//
// The file is compiled once per part (-DRSA_PROBE_PART=0..3), so that the
// template-expanded products compile in parallel and each form takes the
// flags of the production unit that holds it: parts 0-2 (L = 37; L = 74 with
// the modulus in VGPRs; L = 74 with the modulus in SGPRs) with k_rsa_2048's
// flags, part 3 (mont_rt) with k_rsa_big's.
//
// Lane i takes its modulus from the RsaKeyDev row keys[key_idx[i]] (the `u`
// kernels through a wave-uniform index, as rsa_verify_lane<L, true>: every
// live lane of a wave must name the same row), its operands from a[i * L ..]
// and b[i * L ..], and writes n_out words at out[i * n_out ..].  Lanes whose
// `active` byte is zero return at once and leave their results untouched.
#include <hip/hip_runtime.h>

#include "k_rsa.hpp"
#include "rsa_mont.hpp"

#ifndef RSA_PROBE_PART
#error "compile with -DRSA_PROBE_PART=0..3"
#endif

enum { OP_MUL = 0, OP_SQR = 1, OP_CANON = 2, OP_WORDS = 3 };

// entry, L, operation, wave-uniform key row
#define RP_OPS_0(X)              \
  X(mont37, 37, OP_MUL, false)   \
  X(sqr37, 37, OP_SQR, false)    \
  X(mont37u, 37, OP_MUL, true)   \
  X(sqr37u, 37, OP_SQR, true)    \
  X(canon37, 37, OP_CANON, false) \
  X(to_words37, 37, OP_WORDS, false)
#define RP_OPS_1(X)              \
  X(mont74, 74, OP_MUL, false)   \
  X(sqr74, 74, OP_SQR, false)    \
  X(canon74, 74, OP_CANON, false) \
  X(to_words74, 74, OP_WORDS, false)
#define RP_OPS_2(X)              \
  X(mont74u, 74, OP_MUL, true)   \
  X(sqr74u, 74, OP_SQR, true)

struct Args {
  uint32_t n;                // lanes
  const uint8_t* active;     // per lane
  const uint32_t* key_idx;   // per lane
  const RsaKeyDev* keys;
  const uint32_t* a;
  const uint32_t* b;
  uint32_t* out;
  int L;
};

constexpr int words_of(int L) { return (28 * L + 31) / 32; }
constexpr int n_out_of(int L, int op) { return op == OP_WORDS ? words_of(L) : L; }

template <int L, int OP, bool UNI>
__global__ __launch_bounds__(256) void k_fixed(Args g) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n || !g.active[i]) return;
  const uint32_t ki = g.key_idx[i];
  const RsaKeyDev& K = g.keys[UNI ? __builtin_amdgcn_readfirstlane(ki) : ki];
  uint32_t n[L], x[L];
#pragma unroll
  for (int j = 0; j < L; j++) n[j] = K.n28[j], x[j] = g.a[(uint64_t)i * L + j];
  if constexpr (OP == OP_MUL) {
    uint32_t y[L];
#pragma unroll
    for (int j = 0; j < L; j++) y[j] = g.b[(uint64_t)i * L + j];
    mont<L, false>(x, y, n, K.ninv, x);   // out aliases a, as every production call
  }
  if constexpr (OP == OP_SQR) mont<L, true>(x, x, n, K.ninv, x);
  if constexpr (OP == OP_CANON) canon<L>(x, n);
  if constexpr (OP == OP_WORDS) {
    constexpr int W = words_of(L);
    uint32_t w[W];
    to_words<L, W>(x, w);
#pragma unroll
    for (int j = 0; j < W; j++) g.out[(uint64_t)i * W + j] = w[j];
  } else {
#pragma unroll
    for (int j = 0; j < L; j++) g.out[(uint64_t)i * L + j] = x[j];
  }
}

#if RSA_PROBE_PART == 3
// mont_rt at the row's run-time L, arrays in private memory as k_rsa_verify_big
__global__ __launch_bounds__(256) void k_mont_rt(Args g) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n || !g.active[i]) return;
  const RsaKeyDev& K = g.keys[g.key_idx[i]];
  const int L = (int)K.limbs;
  if (L != g.L || L <= 0 || L > RSA_LMAX || L % RSA_BIG_ROWS) return;   // the test builds no such row
  uint32_t x[RSA_LMAX + 1], y[RSA_LMAX + 1], t[RSA_LMAX + 1];
  for (int j = 0; j < L; j++) x[j] = g.a[(uint64_t)i * L + j], y[j] = g.b[(uint64_t)i * L + j];
  rsa_big::mont_rt(x, y, K.n28, K.ninv, L, t);
  for (int j = 0; j <= L; j++) g.out[(uint64_t)i * (L + 1) + j] = t[j];
}
#endif

// hipMalloc, copy in, launch, hipDeviceSynchronize, copy out, free; returns the
// HIP status (or hipErrorInvalidValue for arguments the kernels' bounds
// forbid).  `out` arrives pre-filled by the caller (poison) and is copied in,
// so the results of inactive lanes come back as they went in.
template <typename Kern>
static int run(Kern kern, int L, uint32_t n_out, uint32_t n, const uint8_t* active, const uint32_t* key_idx,
               const uint32_t* keys, uint32_t n_keys, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (n == 0 || n > (1u << 16) || n_keys == 0 || n_keys > (1u << 16) || !active || !key_idx || !keys || !a || !b || !out ||
      L <= 0 || L > RSA_LMAX)
    return (int)hipErrorInvalidValue;
  for (uint32_t i = 0; i < n; i++)
    if (key_idx[i] >= n_keys) return (int)hipErrorInvalidValue;
  const size_t op_b = (size_t)n * L * sizeof(uint32_t), out_b = (size_t)n * n_out * sizeof(uint32_t);
  const size_t key_b = (size_t)n_keys * sizeof(RsaKeyDev);
  uint8_t* d_act = nullptr;
  uint32_t *d_ki = nullptr, *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
  RsaKeyDev* d_keys = nullptr;
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  if (ok(hipMalloc(&d_act, n)) && ok(hipMalloc(&d_ki, n * sizeof(uint32_t))) && ok(hipMalloc(&d_keys, key_b)) &&
      ok(hipMalloc(&d_a, op_b)) && ok(hipMalloc(&d_b, op_b)) && ok(hipMalloc(&d_out, out_b)) &&
      ok(hipMemcpy(d_act, active, n, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_ki, key_idx, n * sizeof(uint32_t), hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_keys, keys, key_b, hipMemcpyHostToDevice)) && ok(hipMemcpy(d_a, a, op_b, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_b, b, op_b, hipMemcpyHostToDevice)) && ok(hipMemcpy(d_out, out, out_b, hipMemcpyHostToDevice))) {
    const Args g{n, d_act, d_ki, d_keys, d_a, d_b, d_out, L};
    hipLaunchKernelGGL(kern, dim3((n + 255) / 256), dim3(256), 0, 0, g);
    if (ok(hipGetLastError()) && ok(hipDeviceSynchronize())) ok(hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost));
  }
  (void)hipFree(d_act);
  (void)hipFree(d_ki);
  (void)hipFree(d_keys);
  (void)hipFree(d_a);
  (void)hipFree(d_b);
  (void)hipFree(d_out);
  return (int)e;
}

extern "C" {
// keys: n_keys rows of RsaKeyDev as uint32 words; L must be the entry's own
#define X(name, LL, OP, UNI)                                                                                         \
  int rp_##name(uint32_t n, const uint8_t* active, const uint32_t* key_idx, const uint32_t* keys, uint32_t n_keys,  \
                const uint32_t* a, const uint32_t* b, uint32_t* out, int L) {                                        \
    if (L != LL) return (int)hipErrorInvalidValue;                                                                   \
    return run(k_fixed<LL, OP, UNI>, LL, n_out_of(LL, OP), n, active, key_idx, keys, n_keys, a, b, out);             \
  }
#if RSA_PROBE_PART == 0
RP_OPS_0(X)
#elif RSA_PROBE_PART == 1
RP_OPS_1(X)
#elif RSA_PROBE_PART == 2
RP_OPS_2(X)
#endif
#undef X

#if RSA_PROBE_PART == 3
// results: L + 1 words per lane (the carry word last)
int rp_mont_rt(uint32_t n, const uint8_t* active, const uint32_t* key_idx, const uint32_t* keys, uint32_t n_keys,
               const uint32_t* a, const uint32_t* b, uint32_t* out, int L) {
  if (L <= 0 || L > RSA_LMAX || L % RSA_BIG_ROWS) return (int)hipErrorInvalidValue;
  return run(k_mont_rt, L, (uint32_t)L + 1, n, active, key_idx, keys, n_keys, a, b, out);
}
#endif

#if RSA_PROBE_PART == 0
// "name:L:results,..." of every entry point of the library (mont_rt: L and
// the result count are the caller's)
const char* rsa_probe_ops() {
  return ""
#define X(name, LL, OP, UNI) #name ":" #LL ":" #OP ","
      RP_OPS_0(X) RP_OPS_1(X) RP_OPS_2(X)
#undef X
      "mont_rt:0:OP_MUL,";
}
int rsa_probe_threads() { return 256; }
int rsa_probe_key_words() { return (int)(sizeof(RsaKeyDev) / sizeof(uint32_t)); }
const char* rsa_probe_error(int status) { return hipGetErrorString((hipError_t)status); }
#endif
}
