// Test-only probe of the one-lane-per-record BLS code (cess_amd/csrc/bls/
// field.hpp Fp and Fp2, curve.hpp, h2c.hpp and the line steps of pairing.hpp,
// the layer behind k_decode_*, k_hash, k_prepare, k_norm_keys, k_sign and
// k_rlc): one small kernel per operation, one lane per row, so that
// tests/test_gpu_lane_primitives.py can compare every primitive with integer
// arithmetic on the operand tables of tests/lane_probe_model.py.  The headers
// are included unchanged; nothing here is linked into libcess_bls.so.
// cess_amd/csrc/Makefile compiles this file once per part (-DLANE_PROBE_PART)
// with the flags of the unit that ships the code: parts 0-3 (field, hash to
// curve) with k_hash's, 4-5 (curve) with k_decode's, 6 (lines) with
// k_prepare's, and links the parts into libcess_lane_probe.so.
//
// Lane i reads n_in words at in[i * n_in ..] and writes n_out words at
// out[i * n_out ..]; the layouts are listed in tests/lane_probe_model.py (an
// Fp is 12 words, an Fp2 c0 then c1, a point x, y, z).  Lanes whose `active`
// byte is zero return at once and leave their results untouched.  The kernels
// take the production block and launch bounds (256 threads, CESS_LB).
//
// soa_layout is the one entry with a layout of its own (soa.hpp's helpers write
// a buffer shared by all lanes): see lp::l_soa_layout.
//
// The lane functions are plain CESS_HD code: the host build
// (tests/hostemu/lane_emu.cpp, -DCESS_HOSTEMU) includes this file and runs the
// same functions in a loop over the lanes.  The two entries of LP_LDS_OPS park
// values in LDS as k_hash and k_prepare do and exist on the device only.
#if !defined(CESS_HOSTEMU)
#include <hip/hip_runtime.h>
#endif

#include "../../cess_amd/csrc/bls/h2c.hpp"
#include "../../cess_amd/csrc/bls/pairing.hpp"
#include "../../cess_amd/csrc/soa.hpp"   // and bls/staged.hpp: lane_fresh, wave_first_thread

#define LP_MSG_WORDS 251   // a message row: length, start offset (0..3), 251 words of bytes
#define LP_N_EXP 7         // pow_fixed's exponents (lp::pow_by_index)
#define LP_LINES 68        // bls::N_COEFFS

// entry, words in, words out, argument check (0 none, 1 message row, 2 exponent index)
#define LP_OPS_0(X)             \
  X(fp_add, 24, 12, 0)          \
  X(fp_sub, 24, 12, 0)          \
  X(fp_add_nr, 24, 12, 0)       \
  X(fp_neg, 12, 12, 0)          \
  X(fp_dbl, 12, 12, 0)          \
  X(fp_mul3, 12, 12, 0)         \
  X(fp_mul4, 12, 12, 0)         \
  X(fp_mul8, 12, 12, 0)         \
  X(fp_reduce_once, 12, 12, 0)  \
  X(fp_is_zero, 12, 1, 0)       \
  X(fp_eq, 24, 1, 0)            \
  X(fp_select, 25, 12, 0)       \
  X(fp_mul, 24, 12, 0)          \
  X(fp_sqr, 12, 12, 0)          \
  X(fp_from_mont, 12, 12, 0)    \
  X(fp_to_mont, 12, 12, 0)      \
  X(fp_pack28, 12, 26, 0)       \
  X(fp_muld_chain, 24, 12, 0)   \
  X(fp_raw_cmp, 12, 2, 0)       \
  X(fp_lex_largest, 12, 1, 0)   \
  X(fp2_add, 48, 24, 0)         \
  X(fp2_sub, 48, 24, 0)         \
  X(fp2_add_nr, 48, 24, 0)      \
  X(fp2_add_xi_nr, 48, 24, 0)   \
  X(fp2_neg, 24, 24, 0)         \
  X(fp2_conj, 24, 24, 0)        \
  X(fp2_mul_nr, 24, 24, 0)      \
  X(fp2_mul, 48, 24, 0)         \
  X(fp2_mul_scaled2, 48, 24, 0) \
  X(fp2_mul_scaled3, 48, 24, 0) \
  X(fp2_dot2, 96, 24, 0)        \
  X(fp2_sqr, 24, 24, 0)         \
  X(fp2_mul_fp, 36, 24, 0)      \
  X(fp2_is_zero, 24, 1, 0)      \
  X(fp2_eq, 48, 1, 0)           \
  X(fp2_lex_largest, 24, 1, 0)
#define LP_OPS_1(X)          \
  X(fp_pow_fixed, 13, 12, 2) \
  X(fp_sqrt, 12, 13, 0)      \
  X(fp_inv, 12, 12, 0)       \
  X(fp2_inv, 24, 24, 0)      \
  X(fp2_sqrt, 24, 25, 0)
#define LP_OPS_2(X)               \
  X(xmd, 253, 32, 1)              \
  X(xmd_select, 253, 32, 1)       \
  X(fp_from_be64_words, 16, 12, 0) \
  X(sgn0, 12, 1, 0)               \
  X(map_to_curve_sswu, 12, 36, 0) \
  X(iso_curve_add, 72, 36, 0)     \
  X(iso_map_proj, 36, 36, 0)      \
  X(clear_cofactor_g1, 24, 25, 0)
#define LP_OPS_3(X) X(hash_to_g1, 253, 25, 1)
#define LP_OPS_4(X)                     \
  X(g1_proj_dbl, 36, 36, 0)             \
  X(g1_proj_add, 72, 36, 0)             \
  X(g1_proj_add_mixed, 60, 36, 0)       \
  X(g1_proj_eq, 72, 1, 0)               \
  X(g1_proj_to_affine, 36, 25, 0)       \
  X(g1_proj_mul_u64, 38, 36, 0)         \
  X(g1_proj_mul_u64_mixed, 26, 36, 0)   \
  X(g1_proj_mul_scalar_mixed, 32, 36, 0) \
  X(sub_r_if_ge, 8, 8, 0)               \
  X(glv_split, 8, 8, 0)                 \
  X(g1_mul_glv, 32, 36, 0)              \
  X(g1_mul_glv32, 26, 36, 0)            \
  X(jac_dbl, 36, 36, 0)                 \
  X(jac_add_mixed, 60, 36, 0)           \
  X(g1_is_torsion_free, 24, 2, 0)       \
  X(g1_decompress, 12, 26, 0)           \
  X(g1_compress, 25, 12, 0)
#define LP_OPS_5(X)                   \
  X(g2_proj_dbl, 72, 72, 0)           \
  X(g2_proj_add, 144, 72, 0)          \
  X(g2_proj_add_mixed, 120, 72, 0)    \
  X(g2_proj_eq, 144, 1, 0)            \
  X(g2_proj_to_affine, 72, 49, 0)     \
  X(g2_proj_mul_u64, 74, 72, 0)       \
  X(g2_proj_mul_u64_mixed, 50, 72, 0) \
  X(g2_is_torsion_free, 48, 1, 0)     \
  X(g2_psi_is_neg_proj, 120, 1, 0)    \
  X(g2_decompress, 25, 50, 0)         \
  X(g2_compress, 49, 24, 0)
#define LP_OPS_6(X)              \
  X(doubling_step, 72, 288, 0)   \
  X(addition_step, 120, 288, 0)  \
  X(normalize_line, 72, 72, 0)   \
  X(normalize_lines, 4896, 6529, 0)
#define LP_OPS_ALL(X) LP_OPS_0(X) LP_OPS_1(X) LP_OPS_2(X) LP_OPS_3(X) LP_OPS_4(X) LP_OPS_5(X) LP_OPS_6(X)
// device only: entry, words in, words out, argument check, part
#define LP_LDS_OPS_3(X) X(hash_to_g1_parked, 253, 25, 1)
#define LP_LDS_OPS_6(X) X(g2_prepare_lds, 48, 4968, 0)
// soa.hpp: words in, words out per lane, words of the shared buffer per column, words of the uniform table
#define LP_SOA_IN 72
#define LP_SOA_OUT 252
#define LP_SOA_SLOT_ROWS 324
#define LP_SOA_TAB 144

namespace lp {
using namespace bls;

CESS_HD fp ldf(const uint32_t* p) {
  fp r;
#pragma unroll
  for (int i = 0; i < 12; i++) r.v[i] = p[i];
  return r;
}
CESS_HD void stf(uint32_t* p, const fp& a) {
#pragma unroll
  for (int i = 0; i < 12; i++) p[i] = a.v[i];
}
CESS_HD fp2 ldf2(const uint32_t* p) { return {ldf(p), ldf(p + 12)}; }
CESS_HD void stf2(uint32_t* p, const fp2& a) { stf(p, a.c0), stf(p + 12, a.c1); }
template <class F> struct Words;
template <> struct Words<fp> { static constexpr int n = 12; };
template <> struct Words<fp2> { static constexpr int n = 24; };
template <class F> CESS_HD F ldF(const uint32_t* p);
template <> CESS_HD fp ldF<fp>(const uint32_t* p) { return ldf(p); }
template <> CESS_HD fp2 ldF<fp2>(const uint32_t* p) { return ldf2(p); }
CESS_HD void stF(uint32_t* p, const fp& a) { stf(p, a); }
CESS_HD void stF(uint32_t* p, const fp2& a) { stf2(p, a); }
template <class F>
CESS_HD proj<F> ldP(const uint32_t* p) {
  constexpr int W = Words<F>::n;
  return {ldF<F>(p), ldF<F>(p + W), ldF<F>(p + 2 * W)};
}
template <class F>
CESS_HD void stP(uint32_t* p, const proj<F>& a) {
  constexpr int W = Words<F>::n;
  stF(p, a.x), stF(p + W, a.y), stF(p + 2 * W, a.z);
}
// inf, x, y
template <class F>
CESS_HD void stA(uint32_t* p, const affine<F>& a) {
  p[0] = a.inf ? 1u : 0u;
  stF(p + 1, a.x), stF(p + 1 + Words<F>::n, a.y);
}
CESS_HD void st_coeff3(uint32_t* p, const coeff3& c) { stf2(p, c.c0), stf2(p + 24, c.c1), stf2(p + 48, c.c2); }
CESS_HD coeff3 ld_coeff3(const uint32_t* p) { return {ldf2(p), ldf2(p + 24), ldf2(p + 48)}; }

// --- Fp ------------------------------------------------------------------------------
CESS_HD void l_fp_add(const uint32_t* in, uint32_t* out) { stf(out, add(ldf(in), ldf(in + 12))); }
CESS_HD void l_fp_sub(const uint32_t* in, uint32_t* out) { stf(out, sub(ldf(in), ldf(in + 12))); }
CESS_HD void l_fp_add_nr(const uint32_t* in, uint32_t* out) { stf(out, add_nr(ldf(in), ldf(in + 12))); }
CESS_HD void l_fp_neg(const uint32_t* in, uint32_t* out) { stf(out, neg(ldf(in))); }
CESS_HD void l_fp_dbl(const uint32_t* in, uint32_t* out) { stf(out, dbl(ldf(in))); }
CESS_HD void l_fp_mul3(const uint32_t* in, uint32_t* out) { stf(out, mul3(ldf(in))); }
CESS_HD void l_fp_mul4(const uint32_t* in, uint32_t* out) { stf(out, mul4(ldf(in))); }
CESS_HD void l_fp_mul8(const uint32_t* in, uint32_t* out) { stf(out, mul8(ldf(in))); }
CESS_HD void l_fp_reduce_once(const uint32_t* in, uint32_t* out) { stf(out, fp_reduce_once(ldf(in))); }
CESS_HD void l_fp_is_zero(const uint32_t* in, uint32_t* out) { out[0] = is_zero(ldf(in)) ? 1u : 0u; }
CESS_HD void l_fp_eq(const uint32_t* in, uint32_t* out) { out[0] = eq(ldf(in), ldf(in + 12)) ? 1u : 0u; }
CESS_HD void l_fp_select(const uint32_t* in, uint32_t* out) { stf(out, select(in[0] != 0, ldf(in + 1), ldf(in + 13))); }
CESS_HD void l_fp_mul(const uint32_t* in, uint32_t* out) { stf(out, mul(ldf(in), ldf(in + 12))); }
CESS_HD void l_fp_sqr(const uint32_t* in, uint32_t* out) { stf(out, sqr(ldf(in))); }
CESS_HD void l_fp_from_mont(const uint32_t* in, uint32_t* out) { stf(out, from_mont(ldf(in))); }
CESS_HD void l_fp_to_mont(const uint32_t* in, uint32_t* out) { stf(out, to_mont(ldf(in))); }
// the 14 digits of unpack28, then pack28 of them
CESS_HD void l_fp_pack28(const uint32_t* in, uint32_t* out) {
  uint32_t d[14];
  unpack28(ldf(in), d);
#pragma unroll
  for (int i = 0; i < 14; i++) out[i] = d[i];
  stf(out + 14, pack28(d));
}
// ((x y)^2 x) in the digit domain, as pow_fixed chains mul_d / sqr_d: x y / R, squared / R, times x / R
CESS_HD void l_fp_muld_chain(const uint32_t* in, uint32_t* out) {
  uint32_t x[14], y[14], t[14];
  unpack28(ldf(in), x);
  unpack28(ldf(in + 12), y);
  mul_d(t, x, y);
  sqr_d(t);
  mul_d(t, t, x);
  stf(out, pack28(t));
}
CESS_HD void l_fp_raw_cmp(const uint32_t* in, uint32_t* out) {
  const fp a = ldf(in);
  out[0] = raw_lt_p(a) ? 1u : 0u;
  out[1] = raw_gt_half(a) ? 1u : 0u;
}
CESS_HD void l_fp_lex_largest(const uint32_t* in, uint32_t* out) { out[0] = lex_largest(ldf(in)) ? 1u : 0u; }

// pow_fixed's exponents: the three the constants keep, then 1, 2^383 + 1, all
// ones and 0x88..8 (a window of every shape; never 0, which pow_fixed does
// not define).  The branch on the index is the caller's: inside one case the
// exponent is the same in every lane, as pow_fixed requires.
CESS_CONST uint32_t EXP_ONE[12] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
CESS_CONST uint32_t EXP_TOP[12] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0x80000000u};
CESS_CONST uint32_t EXP_ONES[12] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu,
                                    0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
CESS_CONST uint32_t EXP_EIGHTS[12] = {0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u,
                                      0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u};
CESS_HD fp pow_by_index(const fp& a, uint32_t idx) {
  switch (idx) {
    case 0: return pow_fixed(a, c::EXP_SQRT);
    case 1: return pow_fixed(a, c::EXP_SQRT_RATIO);
    case 2: return pow_fixed(a, c::EXP_INV);
    case 3: return pow_fixed(a, EXP_ONE);
    case 4: return pow_fixed(a, EXP_TOP);
    case 5: return pow_fixed(a, EXP_ONES);
    default: return pow_fixed(a, EXP_EIGHTS);
  }
}
CESS_HD void l_fp_pow_fixed(const uint32_t* in, uint32_t* out) { stf(out, pow_by_index(ldf(in + 1), in[0])); }
CESS_HD void l_fp_sqrt(const uint32_t* in, uint32_t* out) {
  fp r;
  out[0] = sqrt(r, ldf(in)) ? 1u : 0u;
  stf(out + 1, r);
}
CESS_HD void l_fp_inv(const uint32_t* in, uint32_t* out) { stf(out, inv(ldf(in))); }

// --- Fp2 -----------------------------------------------------------------------------
CESS_HD void l_fp2_add(const uint32_t* in, uint32_t* out) { stf2(out, add(ldf2(in), ldf2(in + 24))); }
CESS_HD void l_fp2_sub(const uint32_t* in, uint32_t* out) { stf2(out, sub(ldf2(in), ldf2(in + 24))); }
CESS_HD void l_fp2_add_nr(const uint32_t* in, uint32_t* out) { stf2(out, add_nr(ldf2(in), ldf2(in + 24))); }
CESS_HD void l_fp2_add_xi_nr(const uint32_t* in, uint32_t* out) { stf2(out, add_xi_nr(ldf2(in), ldf2(in + 24))); }
CESS_HD void l_fp2_neg(const uint32_t* in, uint32_t* out) { stf2(out, neg(ldf2(in))); }
CESS_HD void l_fp2_conj(const uint32_t* in, uint32_t* out) { stf2(out, conj(ldf2(in))); }
CESS_HD void l_fp2_mul_nr(const uint32_t* in, uint32_t* out) { stf2(out, mul_nr(ldf2(in))); }
CESS_HD void l_fp2_mul(const uint32_t* in, uint32_t* out) { stf2(out, mul(ldf2(in), ldf2(in + 24))); }
CESS_HD void l_fp2_mul_scaled2(const uint32_t* in, uint32_t* out) { stf2(out, mul_scaled<2>(ldf2(in), ldf2(in + 24))); }
CESS_HD void l_fp2_mul_scaled3(const uint32_t* in, uint32_t* out) { stf2(out, mul_scaled<3>(ldf2(in), ldf2(in + 24))); }
CESS_HD void l_fp2_dot2(const uint32_t* in, uint32_t* out) {
  stf2(out, dot2(ldf2(in), ldf2(in + 24), ldf2(in + 48), ldf2(in + 72)));
}
CESS_HD void l_fp2_sqr(const uint32_t* in, uint32_t* out) { stf2(out, sqr(ldf2(in))); }
CESS_HD void l_fp2_mul_fp(const uint32_t* in, uint32_t* out) { stf2(out, mul_fp(ldf2(in), ldf(in + 24))); }
CESS_HD void l_fp2_is_zero(const uint32_t* in, uint32_t* out) { out[0] = is_zero(ldf2(in)) ? 1u : 0u; }
CESS_HD void l_fp2_eq(const uint32_t* in, uint32_t* out) { out[0] = eq(ldf2(in), ldf2(in + 24)) ? 1u : 0u; }
CESS_HD void l_fp2_lex_largest(const uint32_t* in, uint32_t* out) { out[0] = lex_largest(ldf2(in)) ? 1u : 0u; }
CESS_HD void l_fp2_inv(const uint32_t* in, uint32_t* out) { stf2(out, inv(ldf2(in))); }
CESS_HD void l_fp2_sqrt(const uint32_t* in, uint32_t* out) {
  fp2 r;
  out[0] = sqrt(r, ldf2(in)) ? 1u : 0u;
  stf2(out + 1, r);
}

// --- hash to curve -------------------------------------------------------------------
CESS_HD const uint8_t* msg_of(const uint32_t* in) { return reinterpret_cast<const uint8_t*>(in + 2) + in[1]; }
CESS_HD void l_xmd(const uint32_t* in, uint32_t* out) {
  uint32_t u[32];
  expand_message_xmd_128<false>(msg_of(in), in[0], u);
#pragma unroll
  for (int i = 0; i < 32; i++) out[i] = u[i];
}
CESS_HD void l_xmd_select(const uint32_t* in, uint32_t* out) {
  uint32_t u[32];
  expand_message_xmd_128<true>(msg_of(in), in[0], u);
#pragma unroll
  for (int i = 0; i < 32; i++) out[i] = u[i];
}
CESS_HD void l_fp_from_be64_words(const uint32_t* in, uint32_t* out) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = in[i];
  stf(out, fp_from_be64_words(w));
}
CESS_HD void l_sgn0(const uint32_t* in, uint32_t* out) { out[0] = sgn0(ldf(in)); }
// xn, xd, y
CESS_HD void l_map_to_curve_sswu(const uint32_t* in, uint32_t* out) {
  fp xn, xd, y;
  map_to_curve_sswu(ldf(in), xn, xd, y);
  stf(out, xn), stf(out + 12, xd), stf(out + 24, y);
}
CESS_HD void l_iso_curve_add(const uint32_t* in, uint32_t* out) { stP(out, iso_curve_add(ldP<fp>(in), ldP<fp>(in + 36))); }
CESS_HD void l_iso_map_proj(const uint32_t* in, uint32_t* out) { stP(out, iso_map_proj(ldf(in), ldf(in + 12), ldf(in + 24))); }
CESS_HD void l_clear_cofactor_g1(const uint32_t* in, uint32_t* out) { stA(out, clear_cofactor_g1(ldf(in), ldf(in + 12))); }
CESS_HD void l_hash_to_g1(const uint32_t* in, uint32_t* out) { stA(out, hash_to_g1(msg_of(in), in[0])); }

// --- curve ---------------------------------------------------------------------------
template <class F> CESS_HD void t_proj_dbl(const uint32_t* in, uint32_t* out) { stP(out, proj_dbl(ldP<F>(in))); }
template <class F> CESS_HD void t_proj_add(const uint32_t* in, uint32_t* out) {
  stP(out, proj_add(ldP<F>(in), ldP<F>(in + 3 * Words<F>::n)));
}
template <class F> CESS_HD void t_proj_add_mixed(const uint32_t* in, uint32_t* out) {
  constexpr int W = Words<F>::n;
  stP(out, proj_add_mixed(ldP<F>(in), ldF<F>(in + 3 * W), ldF<F>(in + 4 * W)));
}
template <class F> CESS_HD void t_proj_eq(const uint32_t* in, uint32_t* out) {
  out[0] = proj_eq(ldP<F>(in), ldP<F>(in + 3 * Words<F>::n)) ? 1u : 0u;
}
template <class F> CESS_HD void t_proj_to_affine(const uint32_t* in, uint32_t* out) { stA(out, proj_to_affine(ldP<F>(in))); }
// the point, then the scalar's low and high word
template <class F> CESS_HD void t_proj_mul_u64(const uint32_t* in, uint32_t* out) {
  constexpr int W = Words<F>::n;
  stP(out, proj_mul_u64(ldP<F>(in), ((uint64_t)in[3 * W + 1] << 32) | in[3 * W]));
}
template <class F> CESS_HD void t_proj_mul_u64_mixed(const uint32_t* in, uint32_t* out) {
  constexpr int W = Words<F>::n;
  stP(out, proj_mul_u64_mixed(ldF<F>(in), ldF<F>(in + W), ((uint64_t)in[2 * W + 1] << 32) | in[2 * W]));
}
#define LP_BOTH(name)                                                                     \
  CESS_HD void l_g1_##name(const uint32_t* in, uint32_t* out) { t_##name<fp>(in, out); }  \
  CESS_HD void l_g2_##name(const uint32_t* in, uint32_t* out) { t_##name<fp2>(in, out); }
LP_BOTH(proj_dbl)
LP_BOTH(proj_add)
LP_BOTH(proj_add_mixed)
LP_BOTH(proj_eq)
LP_BOTH(proj_to_affine)
LP_BOTH(proj_mul_u64)
LP_BOTH(proj_mul_u64_mixed)
#undef LP_BOTH

template <int N>
CESS_HD void ldw(const uint32_t* p, uint32_t (&w)[N]) {
#pragma unroll
  for (int i = 0; i < N; i++) w[i] = p[i];
}
CESS_HD void l_g1_proj_mul_scalar_mixed(const uint32_t* in, uint32_t* out) {
  uint32_t k[8];
  ldw(in + 24, k);
  stP(out, proj_mul_scalar_mixed(ldf(in), ldf(in + 12), k));
}
CESS_HD void l_sub_r_if_ge(const uint32_t* in, uint32_t* out) {
  uint32_t k[8];
  ldw(in, k);
  sub_r_if_ge(k);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = k[i];
}
// k1, k2
CESS_HD void l_glv_split(const uint32_t* in, uint32_t* out) {
  uint32_t k[8], k1[4], k2[4];
  ldw(in, k);
  glv_split(k, k1, k2);
#pragma unroll
  for (int i = 0; i < 4; i++) out[i] = k1[i], out[4 + i] = k2[i];
}
CESS_HD void l_g1_mul_glv(const uint32_t* in, uint32_t* out) {
  uint32_t k[8];
  ldw(in + 24, k);
  stP(out, g1_mul_glv(ldf(in), ldf(in + 12), k));
}
CESS_HD void l_g1_mul_glv32(const uint32_t* in, uint32_t* out) {
  stP(out, g1_mul_glv32(ldf(in), ldf(in + 12), in[24], in[25]));
}
CESS_HD void l_jac_dbl(const uint32_t* in, uint32_t* out) { stP(out, jac_dbl(ldP<fp>(in))); }
CESS_HD void l_jac_add_mixed(const uint32_t* in, uint32_t* out) {
  stP(out, jac_add_mixed(ldP<fp>(in), ldf(in + 36), ldf(in + 48)));
}
// the Jacobian form, the complete-formula form
CESS_HD void l_g1_is_torsion_free(const uint32_t* in, uint32_t* out) {
  const fp x = ldf(in), y = ldf(in + 12);
  out[0] = g1_is_torsion_free(x, y) ? 1u : 0u;
  out[1] = g1_is_torsion_free_rcb(x, y) ? 1u : 0u;
}
CESS_HD void l_g2_is_torsion_free(const uint32_t* in, uint32_t* out) {
  out[0] = g2_is_torsion_free(ldf2(in), ldf2(in + 24), RegPark2{}) ? 1u : 0u;
}
CESS_HD void l_g2_psi_is_neg_proj(const uint32_t* in, uint32_t* out) {
  out[0] = g2_psi_is_neg_proj(ldf2(in), ldf2(in + 24), ldf2(in + 48), ldf2(in + 72), ldf2(in + 96)) ? 1u : 0u;
}
// in: the 12 big-endian words of the encoding; out: valid, inf, x, y
CESS_HD void l_g1_decompress(const uint32_t* in, uint32_t* out) {
  uint32_t w[12];
  ldw(in, w);
  g1a a;
  out[0] = g1_decompress(w, a) ? 1u : 0u;
  stA(out + 1, a);
}
// in: subgroup, the 24 big-endian words; out: valid, inf, x, y
CESS_HD void l_g2_decompress(const uint32_t* in, uint32_t* out) {
  uint32_t w[24];
  ldw(in + 1, w);
  g2a a;
  out[0] = g2_decompress(w, a, RegPark2{}, in[0] != 0) ? 1u : 0u;
  stA(out + 1, a);
}
// in: inf, x, y; out: the encoding's bytes, four to a word, first byte lowest
template <int N>
CESS_HD void st_bytes(uint32_t* out, const uint8_t (&b)[N]) {
#pragma unroll
  for (int i = 0; i < N / 4; i++)
    out[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}
CESS_HD void l_g1_compress(const uint32_t* in, uint32_t* out) {
  g1a a;
  a.inf = in[0] != 0, a.x = ldf(in + 1), a.y = ldf(in + 13);
  uint8_t b[48];
  g1_compress(a, b);
  st_bytes(out, b);
}
CESS_HD void l_g2_compress(const uint32_t* in, uint32_t* out) {
  g2a a;
  a.inf = in[0] != 0, a.x = ldf2(in + 1), a.y = ldf2(in + 25);
  uint8_t b[96];
  g2_compress(a, b);
  st_bytes(out, b);
}

// --- line steps ----------------------------------------------------------------------
// out: the value-returning step's c0, c1, c2 and new R, then the emit form's
CESS_HD void l_doubling_step(const uint32_t* in, uint32_t* out) {
  g2p r = ldP<fp2>(in);
  st_coeff3(out, doubling_step(r));
  stP(out + 72, r);
  r = ldP<fp2>(in);
  doubling_step_emit(r, 0, [&](int, int j, const fp2& c) { stf2(out + 144 + 24 * j, c); });
  stP(out + 216, r);
}
// in: R, then the affine Q
CESS_HD void l_addition_step(const uint32_t* in, uint32_t* out) {
  g2p r = ldP<fp2>(in);
  st_coeff3(out, addition_step(r, ldf2(in + 72), ldf2(in + 96)));
  stP(out + 72, r);
  r = ldP<fp2>(in);
  addition_step_emit(
      r, [&](fp2& x, fp2& y) { x = ldf2(in + 72), y = ldf2(in + 96); }, 0,
      [&](int, int j, const fp2& c) { stf2(out + 144 + 24 * j, c); });
  stP(out + 216, r);
}
CESS_HD void l_normalize_line(const uint32_t* in, uint32_t* out) {
  coeff3 k = ld_coeff3(in);
  normalize_line(k);
  st_coeff3(out, k);
}
// in: 68 lines; out: the flag, the 68 lines as normalize_lines left them, its 68 Fp2 of scratch
CESS_HD void l_normalize_lines(const uint32_t* in, uint32_t* out) {
  uint32_t* tab = out + 1;
  uint32_t* pre = out + 1 + 72 * LP_LINES;
#pragma unroll 1
  for (int i = 0; i < 72 * LP_LINES; i++) tab[i] = in[i];
  const bool ok = normalize_lines([&](int k) { return ld_coeff3(tab + 72 * k); },
                                  [&](int k, const coeff3& c) { st_coeff3(tab + 72 * k, c); },
                                  [&](int k) { return ldf2(pre + 24 * k); }, [&](int k, const fp2& v) { stf2(pre + 24 * k, v); });
  out[0] = ok ? 1u : 0u;
}

// soa.hpp.  in: a coefficient triple c (72 words).  slots: 324 rows of `stride`
// words (stride >= n), lane i owning column i -- rows 0..11 st_fp of c0.c0,
// rows 12..35 st_fp2 of c1, then two uint4-row tables of 2 lines (36 uint4 rows
// = 144 word rows each): st_coeff4 of c as line 1 of the first, st_coeff4_one
// of c0, c1, c2 as line 1 of the second; line 0 of both stays as it came.
// out: ld_fp, ld_fp2, ld_coeff4 of both tables' line 1, and ld_coeff_uniform
// of line (i & 1) of the 2-line table `tab`.
CESS_HD void l_soa_layout(uint32_t i, uint64_t stride, const uint32_t* in, uint32_t* slots, const uint32_t* tab, uint32_t* out) {
  using namespace cess;
  const coeff3 c = ld_coeff3(in);
  uint32_t* A = slots;
  uint32_t* B = slots + 12 * stride;
  uint4* C = reinterpret_cast<uint4*>(slots + 36 * stride);
  uint4* D = reinterpret_cast<uint4*>(slots + 180 * stride);
  st_fp(A, stride, i, c.c0.c0);
  st_fp2(B, stride, i, c.c1);
  st_coeff4(C, stride, i, 1, c);
  st_coeff4_one(D, stride, i, 1, 0, c.c0);
  st_coeff4_one(D, stride, i, 1, 1, c.c1);
  st_coeff4_one(D, stride, i, 1, 2, c.c2);
  CESS_MEMBAR();
  stf(out, ld_fp(A, stride, i));
  stf2(out + 12, ld_fp2(B, stride, i));
  st_coeff3(out + 36, ld_coeff4(C, stride, i, 1));
  st_coeff3(out + 108, ld_coeff4(D, stride, i, 1));
  st_coeff3(out + 180, ld_coeff_uniform(tab, (int)(i & 1u)));
}
inline bool soa_args_ok(uint32_t n, uint32_t stride, const uint8_t* active, const uint32_t* in, const uint32_t* slots,
                        const uint32_t* tab, const uint32_t* out) {
  return n != 0 && n <= (1u << 16) && stride >= n && stride <= (1u << 17) && active && in && slots && tab && out;
}

#if !defined(CESS_HOSTEMU)
// hash_to_g1_parked as k_hash calls it: the block's park, the lane's thread index
CESS_HD void l_hash_to_g1_parked(const uint32_t* in, uint32_t* out, uint32_t (*park)[256], uint32_t t) {
  stA(out, hash_to_g1_parked(msg_of(in), in[0], park, t));
}
// g2_prepare_emit with the key parked in LDS and re-read at the addition steps
// through the wave's first thread plus the lane's number, as k_prepare reads
// it.  in: the affine Q; out: the 68 lines, then T = [|x|]Q
CESS_HD void l_g2_prepare_lds(const uint32_t* in, uint32_t* out, uint4 (*QP)[256], uint32_t t0) {
  {
    const fp2 qx = ldf2(in), qy = ldf2(in + 24);
#pragma unroll
    for (int w = 0; w < 6; w++) {
      const fp& a = w < 3 ? qx.c0 : qx.c1;
      QP[w][t0] = make_uint4(a.v[4 * (w % 3)], a.v[4 * (w % 3) + 1], a.v[4 * (w % 3) + 2], a.v[4 * (w % 3) + 3]);
      const fp& b = w < 3 ? qy.c0 : qy.c1;
      QP[6 + w][t0] = make_uint4(b.v[4 * (w % 3)], b.v[4 * (w % 3) + 1], b.v[4 * (w % 3) + 2], b.v[4 * (w % 3) + 3]);
    }
  }
  const uint32_t w0 = wave_first_thread();
  auto q = [&](fp2& x, fp2& y) {
    const uint32_t t = w0 + lane_fresh();
#pragma unroll
    for (int w = 0; w < 6; w++) {
      const uint4 a = QP[w][t], b = QP[6 + w][t];
      fp& da = w < 3 ? x.c0 : x.c1;
      fp& db = w < 3 ? y.c0 : y.c1;
      const int o = 4 * (w % 3);
      da.v[o] = a.x, da.v[o + 1] = a.y, da.v[o + 2] = a.z, da.v[o + 3] = a.w;
      db.v[o] = b.x, db.v[o + 1] = b.y, db.v[o + 2] = b.z, db.v[o + 3] = b.w;
    }
  };
  const g2p t = g2_prepare_emit(q, [&](int k, int j, const fp2& c) { stf2(out + 72 * k + 24 * j, c); });
  stP(out + 72 * LP_LINES, t);
}
#endif

// what the lanes' bounds forbid: a lane count outside [1, 2^16], a missing
// array, a message that leaves its row, an exponent index outside the list
inline bool args_ok(uint32_t n_in, int check, uint32_t n, const uint8_t* active, const uint32_t* in, const uint32_t* out) {
  if (n == 0 || n > (1u << 16) || !active || !in || !out) return false;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t* row = in + (uint64_t)i * n_in;
    if (check == 1 && (row[1] > 3 || row[0] > 4 * LP_MSG_WORDS - row[1])) return false;
    if (check == 2 && row[0] >= LP_N_EXP) return false;
  }
  return true;
}

}  // namespace lp

#if !defined(CESS_HOSTEMU)
#ifndef LANE_PROBE_PART
#error "compile with -DLANE_PROBE_PART=0..6"
#endif

struct LpArgs {
  uint32_t n;              // lanes
  const uint8_t* active;   // per lane
  const uint32_t* in;
  uint32_t* out;
};

#if LANE_PROBE_PART == 0
#define LP_OPS_HERE(X) LP_OPS_0(X)
#elif LANE_PROBE_PART == 1
#define LP_OPS_HERE(X) LP_OPS_1(X)
#elif LANE_PROBE_PART == 2
#define LP_OPS_HERE(X) LP_OPS_2(X)
#elif LANE_PROBE_PART == 3
#define LP_OPS_HERE(X) LP_OPS_3(X)
#elif LANE_PROBE_PART == 4
#define LP_OPS_HERE(X) LP_OPS_4(X)
#elif LANE_PROBE_PART == 5
#define LP_OPS_HERE(X) LP_OPS_5(X)
#elif LANE_PROBE_PART == 6
#define LP_OPS_HERE(X) LP_OPS_6(X)
#endif

#define X(name, NI, NO, CHK)                                           \
  __global__ CESS_LB void k_lp_##name(LpArgs g) {                      \
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;          \
    if (i >= g.n || !g.active[i]) return;                              \
    lp::l_##name(g.in + (uint64_t)i * NI, g.out + (uint64_t)i * NO);   \
  }
LP_OPS_HERE(X)
#undef X

#if LANE_PROBE_PART == 3
__global__ CESS_LB void k_lp_hash_to_g1_parked(LpArgs g) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n || !g.active[i]) return;
  __shared__ uint32_t park[48][256];   // 48 KiB per block, as k_hash
  lp::l_hash_to_g1_parked(g.in + (uint64_t)i * 253, g.out + (uint64_t)i * 25, park, threadIdx.x);
}
#endif
#if LANE_PROBE_PART == 6
__global__ CESS_LB void k_lp_g2_prepare_lds(LpArgs g) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n || !g.active[i]) return;
  __shared__ uint4 QP[12][256];   // 48 KiB per block, as k_prepare
  lp::l_g2_prepare_lds(g.in + (uint64_t)i * 48, g.out + (uint64_t)i * 4968, QP, threadIdx.x);
}
#endif

#if LANE_PROBE_PART == 6
__global__ CESS_LB void k_lp_soa_layout(LpArgs g, uint32_t stride, uint32_t* slots, const uint32_t* tab) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n || !g.active[i]) return;
  lp::l_soa_layout(i, stride, g.in + (uint64_t)i * LP_SOA_IN, slots, tab, g.out + (uint64_t)i * LP_SOA_OUT);
}
#endif

// hipMalloc, copy in, launch, hipDeviceSynchronize, copy out, free; returns the
// HIP status (or hipErrorInvalidValue for arguments the lanes' bounds forbid).
// `out` arrives pre-filled by the caller (poison) and is copied in, so the
// results of inactive lanes come back as they went in.
template <typename Kern>
static int lp_run(Kern kern, uint32_t n_in, uint32_t n_out, int check, uint32_t n, const uint8_t* active, const uint32_t* in,
                  uint32_t* out) {
  if (!lp::args_ok(n_in, check, n, active, in, out)) return (int)hipErrorInvalidValue;
  const size_t in_b = (size_t)n * n_in * sizeof(uint32_t), out_b = (size_t)n * n_out * sizeof(uint32_t);
  uint8_t* d_act = nullptr;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  if (ok(hipMalloc(&d_act, n)) && ok(hipMalloc(&d_in, in_b)) && ok(hipMalloc(&d_out, out_b)) &&
      ok(hipMemcpy(d_act, active, n, hipMemcpyHostToDevice)) && ok(hipMemcpy(d_in, in, in_b, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_out, out, out_b, hipMemcpyHostToDevice))) {
    const LpArgs g{n, d_act, d_in, d_out};
    hipLaunchKernelGGL(kern, dim3((n + 255) / 256), dim3(256), 0, 0, g);
    if (ok(hipGetLastError()) && ok(hipDeviceSynchronize())) ok(hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost));
  }
  (void)hipFree(d_act);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return (int)e;
}

extern "C" {
#define X(name, NI, NO, CHK)                                                             \
  int lp_##name(uint32_t n, const uint8_t* active, const uint32_t* in, uint32_t* out) { \
    return lp_run(k_lp_##name, NI, NO, CHK, n, active, in, out);                         \
  }
LP_OPS_HERE(X)
#if LANE_PROBE_PART == 3
LP_LDS_OPS_3(X)
#endif
#if LANE_PROBE_PART == 6
LP_LDS_OPS_6(X)
#endif
#undef X

#if LANE_PROBE_PART == 6
// slots (324 * stride words) and out arrive pre-filled by the caller and are
// copied in and back, so that what no live lane wrote comes back as it went in
int lp_soa_layout(uint32_t n, uint32_t stride, const uint8_t* active, const uint32_t* in, uint32_t* slots, const uint32_t* tab,
                  uint32_t* out) {
  if (!lp::soa_args_ok(n, stride, active, in, slots, tab, out)) return (int)hipErrorInvalidValue;
  const size_t in_b = (size_t)n * LP_SOA_IN * 4, out_b = (size_t)n * LP_SOA_OUT * 4;
  const size_t slot_b = (size_t)LP_SOA_SLOT_ROWS * stride * 4, tab_b = (size_t)LP_SOA_TAB * 4;
  uint8_t* d_act = nullptr;
  uint32_t *d_in = nullptr, *d_out = nullptr, *d_slots = nullptr, *d_tab = nullptr;
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  if (ok(hipMalloc(&d_act, n)) && ok(hipMalloc(&d_in, in_b)) && ok(hipMalloc(&d_out, out_b)) && ok(hipMalloc(&d_slots, slot_b)) &&
      ok(hipMalloc(&d_tab, tab_b)) && ok(hipMemcpy(d_act, active, n, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_in, in, in_b, hipMemcpyHostToDevice)) && ok(hipMemcpy(d_out, out, out_b, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_slots, slots, slot_b, hipMemcpyHostToDevice)) && ok(hipMemcpy(d_tab, tab, tab_b, hipMemcpyHostToDevice))) {
    const LpArgs g{n, d_act, d_in, d_out};
    hipLaunchKernelGGL(k_lp_soa_layout, dim3((n + 255) / 256), dim3(256), 0, 0, g, stride, d_slots, d_tab);
    if (ok(hipGetLastError()) && ok(hipDeviceSynchronize()) && ok(hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost)))
      ok(hipMemcpy(slots, d_slots, slot_b, hipMemcpyDeviceToHost));
  }
  (void)hipFree(d_act);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  (void)hipFree(d_slots);
  (void)hipFree(d_tab);
  return (int)e;
}
#endif

#if LANE_PROBE_PART == 0
// "name:words in:words out,..." of every entry point of the library
const char* lane_probe_ops() {
  return ""
#define X(name, NI, NO, CHK) #name ":" #NI ":" #NO ","
      LP_OPS_ALL(X) LP_LDS_OPS_3(X) LP_LDS_OPS_6(X)
#undef X
      "soa_layout:72:252,";
}
int lane_probe_threads() { return 256; }
const char* lane_probe_error(int status) { return hipGetErrorString((hipError_t)status); }
#endif
}
#endif
