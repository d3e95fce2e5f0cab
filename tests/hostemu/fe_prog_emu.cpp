// TEST HARNESS ONLY: the two final-exponentiation programs of bls/staged.hpp
// (CESS_FE_PROGRAM with Gt output, CESS_FE_PROGRAM_VERIFY verdict only) run
// separately on one record's Miller value, compiled for the host
// (CESS_HOSTEMU), and their opcode counts.  Never linked into the product
// library.  (emu.cpp's emu_verify folds the two verdicts into one code.)
#include <string.h>
#include "../../cess_amd/csrc/bls/h2c.hpp"
#include "../../cess_amd/csrc/bls/staged.hpp"

using namespace bls;

static const uint8_t kProg[][2] = {CESS_FE_PROGRAM};
static const uint8_t kProgVerify[][2] = {CESS_FE_PROGRAM_VERIFY};

static void be_words(const uint8_t* b, int nwords, uint32_t* w) {
  for (int i = 0; i < nwords; i++)
    w[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
}

static coeff3 g_neg_g2[N_COEFFS];
static bool g_init = false;
static void init_neg_g2() {
  if (g_init) return;
  fp2 gx = {fp_from(c::G2_GEN_X0), fp_from(c::G2_GEN_X1)};
  fp2 gy = neg(fp2{fp_from(c::G2_GEN_Y0), fp_from(c::G2_GEN_Y1)});
  g2_prepare(gx, gy, [](int i, const coeff3& k) { g_neg_g2[i] = k; });
  for (int i = 0; i < N_COEFFS; i++) normalize_line(g_neg_g2[i]);   // as the device table (k_norm_lines)
  g_init = true;
}

extern "C" {
// occurrences of opcode `op` (FeOp) in the Gt-output program (verify = 0) or
// the verdict-only program (verify = 1); op < 0: the program's length
// without FE_END.  sqn = 1: the sum of FE_SQN's arguments instead.
int emu_fe_prog_count(int verify, int op, int sqn) {
  const uint8_t(*p)[2] = verify ? kProgVerify : kProg;
  int n = 0;
  for (int pc = 0; p[pc][0] != FE_END; pc++) {
    if (op < 0) n++;
    else if (p[pc][0] == op) n += sqn ? p[pc][1] : 1;
  }
  return n;
}
int emu_fe_slot_count() { return SL_N; }
}

static fp12 g_slots[SL_N], g_acc, g_acc1, g_park;
// the staged Miller loop's value for (sig, msg, pk) into g_slots[SL_F]; 2 / 4
// when the signature / key does not decode, else 0
static int miller_value(const uint8_t* sig, const uint8_t* msg, uint32_t mlen, const uint8_t* pk) {
  init_neg_g2();
  uint32_t ws[12], wp[24];
  be_words(sig, 12, ws);
  be_words(pk, 24, wp);
  g1a s;
  if (!g1_decompress(ws, s)) return 2;
  g2a q;
  if (!g2_decompress(wp, q)) return 4;
  static g1a pts[2];
  pts[0] = s;
  pts[1] = hash_to_g1(msg, mlen);
  static coeff3 pkc[N_COEFFS];
  fp2 qx = q.inf ? fp2{fp_from(c::G2_GEN_X0), fp_from(c::G2_GEN_X1)} : q.x;
  fp2 qy = q.inf ? fp2{fp_from(c::G2_GEN_Y0), fp_from(c::G2_GEN_Y1)} : q.y;
  g2_prepare(qx, qy, [](int i, const coeff3& k) { pkc[i] = k; });
  miller_loop2_staged(ArrF12{&g_slots[SL_F]}, !s.inf, !(q.inf || pts[1].inf), [](int pair) { return pts[pair]; },
                      [](int pair, int i) { return pair ? pkc[i] : g_neg_g2[i]; });
  return 0;
}
// one program on g_slots[SL_F]; returns the accumulator holding the result
static const fp12& run_program(const uint8_t (*prog)[2]) {
  const int w = final_exp_staged(ArrF12{&g_acc}, ArrF12{&g_acc1}, prog, [](int sl) { return ArrF12{&g_slots[sl]}; },
                                 ArrF12{&g_park});
  return w ? g_acc1 : g_acc;
}

extern "C" {
// Both programs on the Miller value of (sig, msg, pk).  Returns 2 / 4 when the
// signature / key does not decode, else 0 with
//   *code_full   = 0 if the Gt-output program's result is one, else 5,
//   *code_verify = 0 if the verdict-only program accepts (its accumulator
//                  equals conj(SL_T4), as the kernels compare), else 5,
//   gt_out       = the Gt-output program's 576 bytes.
int emu_fe_both(const uint8_t* sig, const uint8_t* msg, uint32_t mlen, const uint8_t* pk, int* code_full,
                int* code_verify, uint8_t* gt_out) {
  const int st = miller_value(sig, msg, mlen, pk);
  if (st) return st;
  const fp12 f = g_slots[SL_F];
  const fp12 g = run_program(kProg);
  const fp* e = &g.c0.c0.c0;
  for (int i = 0; i < 12; i++) raw_to_be48(from_mont(e[i]), gt_out + 48 * i);
  *code_full = is_one(g) ? 0 : 5;
  // fresh slots: nothing the first program left may decide the second
  memset(g_slots, 0, sizeof(g_slots));
  g_slots[SL_F] = f;
  const fp12& v = run_program(kProgVerify);
  *code_verify = is_conj12(ArrF12{const_cast<fp12*>(&v)}, ArrF12{&g_slots[SL_T4]}) ? 0 : 5;
  return 0;
}

#if defined(CESS_COUNT_OPS)
// (half-multiply, square) counts (as emu.cpp emu_opcount) of one program on the
// record's Miller value: verify = 1 the verdict-only program with its
// comparison (what k_final / k_final2 run per signature), 0 the Gt-output one
void emu_fe_opcount(const uint8_t* sig, const uint8_t* msg, uint32_t mlen, const uint8_t* pk, int verify,
                    uint64_t* out) {
  out[0] = out[1] = 0;
  if (miller_value(sig, msg, mlen, pk)) return;
  g_mul_count = g_sqr_count = g_mul2_count = g_half_count = 0;
  const fp12& v = run_program(verify ? kProgVerify : kProg);
  if (verify) (void)is_conj12(ArrF12{const_cast<fp12*>(&v)}, ArrF12{&g_slots[SL_T4]});
  out[0] = 2 * g_mul_count + 5 * g_mul2_count + g_half_count;
  out[1] = g_sqr_count;
}
#endif
}
