// Probe of the Montgomery column code generation: one bls::mul and one
// bls::sqr per thread, nothing else.  tests/test_column_chain.py compiles it
// with the flags the Makefile gives k_decode and counts v_lshl_add_u64 (one
// per column when the compiler splits a column's sum off the carried chain)
// and v_mad_u64_u32.  Elements are addressed by threadIdx.x alone, so the
// loads and stores take the SGPR-base + 32-bit-offset form and the kernels
// hold no 64-bit address adds of their own.
#include <hip/hip_runtime.h>
#include "bls/field.hpp"

using namespace bls;

__global__ void k_probe_mul(const fp* __restrict__ a, const fp* __restrict__ b, fp* __restrict__ r) {
  const uint32_t i = threadIdx.x;
  r[i] = mul(a[i], b[i]);
}

__global__ void k_probe_sqr(const fp* __restrict__ a, fp* __restrict__ r) {
  const uint32_t i = threadIdx.x;
  r[i] = sqr(a[i]);
}
