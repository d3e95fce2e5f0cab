// Test-only probe of the lane-group layer (cess_amd/csrc/bls/group.hpp, run by
// k_group and k_group_fe of k_group.hip): the half-products grp_mul_comp and
// grp_sqr_comp alone, one round of a lane-group program on a caller-built
// register file, and the two shipped kernels on caller-built inputs, so that
// tests/test_gpu_group_primitives.py can compare each with integer arithmetic
// on the tables of tests/group_probe_model.py.  k_group.hip, bls/group.hpp and
// both program headers are included unchanged (the probe takes the kernel's
// Regs and the two kernels themselves from k_group.hip); nothing here is
// linked into libcess_bls.so.  cess_amd/csrc/Makefile builds it with k_group's
// flags into libcess_group_probe.so.
//
// Entries (words per row in, words per row out; gp_ops):
//   grp_mul_comp 48 -> 24   a row is an operand pair A, B (Fp2 each, c0 then
//   grp_sqr_comp 24 -> 24   c1, 12 raw words a component, as the register file
//                           holds them); lane 2 row + comp computes component
//                           comp, so both components of a row sit in
//                           neighbouring lanes, as in the kernel.
//   round       129 -> 0    one wave per row: a header word (kind | count << 8
//                           | first entry << 16) and 32 sixteen-byte entries;
//                           the row's register-file image (n_slots x 24 words,
//                           n_slots <= grp::N_SLOTS) is loaded into LDS, ONE
//                           round runs, and the whole image is written back.
//   group_fe    144 -> 145  the shipped k_group_fe: uint4 SoA of stride m in,
//                           576 Gt bytes and the code out.
//   group        96 -> 145  the shipped k_group: code / inf / code2 / inf2
//                           bytes and SoA affine arrays of a stride >= n in.
// Rows whose `active` byte is zero return at once (mul, sqr, round).
//
// k_gp_round runs the kernels' own loop, group_rounds of k_group.hip (the one
// function k_group and k_group_fe call: the lane assignment op = lane >> 1,
// comp = lane & 1, the header and entry prefetch with idle lanes op >= cnt,
// group_eval_comp, Regs::st_comp after the reads, the barrier), on a program
// of one round.
//
// The lane functions and argument checks are plain CESS_HD / host code: the
// host build (tests/hostemu/group_probe_emu.cpp, -DCESS_HOSTEMU) includes this
// file and runs them in loops with read-before-write rounds.
#if !defined(CESS_HOSTEMU)
#include "../../cess_amd/csrc/k_group.hip"
#else
#include "../../cess_amd/csrc/bls/group.hpp"
#include "../../cess_amd/csrc/bls/group_fe_prog.hpp"
#endif

#define GP_MUL_IN 48
#define GP_SQR_IN 24
#define GP_COMP_OUT 12     // per lane; 24 per row
#define GP_ROUND_ENTS 32   // entries of a row's round
#define GP_MAX_ROWS 4096u
#define GP_OPS_STRING "grp_mul_comp:48:24,grp_sqr_comp:24:24,round:129:0,group_fe:144:145,group:96:145,"

namespace gp {
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

// in: the row's operands; out: this lane's 12 words
CESS_HD void l_grp_mul_comp(const uint32_t* in, uint32_t* out, uint32_t comp) {
  stf(out, grp_mul_comp(ldf2(in), ldf2(in + 24), comp));
}
CESS_HD void l_grp_sqr_comp(const uint32_t* in, uint32_t* out, uint32_t comp) { stf(out, grp_sqr_comp(ldf2(in), comp)); }

inline bool comp_args_ok(uint32_t lanes, const uint8_t* active, const uint32_t* in, const uint32_t* out) {
  return lanes != 0 && (lanes & 1u) == 0 && lanes <= 2 * GP_MAX_ROWS && active && in && out;
}

// what one round may touch: every slot index it names lies below n_slots,
// every constant index inside the pool, the entries inside the row's 32
inline bool round_ok(uint32_t n_slots, uint32_t head, const uint32_t* ents) {
  const uint32_t kind = head & 0xffu, cnt = (head >> 8) & 0xffu, off = head >> 16;
  if (kind > GRP_INV || cnt > 32 || off + cnt > GP_ROUND_ENTS) return false;
  for (uint32_t k = 0; k < cnt; k++) {
    const uint32_t* e = ents + 4 * (off + k);
    auto byte = [&](uint32_t p) { return (e[p >> 2] >> (8 * (p & 3))) & 0xffu; };
    if (byte(0) >= n_slots) return false;
    if (kind == GRP_MUL || kind == GRP_SQR) {
      const uint32_t f = byte(5);
      if (byte(1) >= ((f & 16) ? (uint32_t)grp::N_CONSTS : n_slots)) return false;
      if ((f & 1) && byte(2) >= n_slots) return false;
      if (kind == GRP_MUL) {
        if (byte(3) >= ((f & 32) ? (uint32_t)grp::N_CONSTS : n_slots)) return false;
        if ((f & 4) && byte(4) >= n_slots) return false;
      }
    } else if (kind == GRP_LIN) {
      const uint32_t terms = (byte(1) & 15u) + (byte(1) >> 4) + (byte(2) & 15u) + (byte(2) >> 4);
      if (terms > 12) return false;
      for (uint32_t t = 0; t < terms; t++)
        if (byte(3 + t) >= n_slots) return false;
    } else if (byte(1) >= n_slots) {
      return false;
    }
  }
  return true;
}
inline bool round_args_ok(uint32_t n, uint32_t n_slots, const uint8_t* active, const uint32_t* heads, const uint32_t* ents,
                          const uint32_t* img) {
  if (n == 0 || n > GP_MAX_ROWS || n_slots == 0 || n_slots > (uint32_t)grp::N_SLOTS || !active || !heads || !ents || !img)
    return false;
  for (uint32_t i = 0; i < n; i++)
    if (!round_ok(n_slots, heads[i], ents + (uint64_t)i * 4 * GP_ROUND_ENTS)) return false;
  return true;
}

}  // namespace gp

#if !defined(CESS_HOSTEMU)

__global__ __launch_bounds__(64) void k_gp_mul_comp(uint32_t lanes, const uint8_t* active, const uint32_t* in, uint32_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= lanes || !active[i >> 1]) return;
  gp::l_grp_mul_comp(in + (uint64_t)(i >> 1) * GP_MUL_IN, out + (uint64_t)i * GP_COMP_OUT, i & 1u);
}
__global__ __launch_bounds__(64) void k_gp_sqr_comp(uint32_t lanes, const uint8_t* active, const uint32_t* in, uint32_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= lanes || !active[i >> 1]) return;
  gp::l_grp_sqr_comp(in + (uint64_t)(i >> 1) * GP_SQR_IN, out + (uint64_t)i * GP_COMP_OUT, i & 1u);
}

// One block (one wave) per row, as k_group: the row's image into the LDS
// register file, one round, the image back.
__global__ __launch_bounds__(64) void k_gp_round(uint32_t n, const uint8_t* active, uint32_t n_slots, const uint32_t* heads,
                                                 const uint4* ents_all, uint4* img) {
  const uint32_t i = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  if (i >= n || !active[i]) return;
  __shared__ uint4 S[grp::N_SLOTS][6];
  const Regs R{S};
  uint4* g = img + (uint64_t)i * 6 * n_slots;
  for (uint32_t q = lane; q < 6 * n_slots; q += 64) S[q / 6][q % 6] = g[q];
  __syncthreads();
  group_rounds(R, heads + i, 1, ents_all + (uint64_t)i * GP_ROUND_ENTS, lane);   // (ends on its barrier)
  for (uint32_t q = lane; q < 6 * n_slots; q += 64) g[q] = S[q / 6][q % 6];
}

namespace {
// device buffers of one call: the first error sticks, everything is freed
struct Dev {
  hipError_t e = hipSuccess;
  void* p[12];
  int np = 0;
  bool ok(hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  }
  template <class T>
  T* up(const T* host, size_t bytes) {   // hipMalloc + copy in (host may be null: no buffer)
    if (!host || e != hipSuccess) return nullptr;
    void* d = nullptr;
    if (!ok(hipMalloc(&d, bytes))) return nullptr;
    p[np++] = d;
    ok(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
    return static_cast<T*>(d);
  }
  template <class T>
  void down(T* host, const T* dev, size_t bytes) {
    if (e == hipSuccess) ok(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
  }
  bool ran() { return ok(hipGetLastError()) && ok(hipDeviceSynchronize()); }
  ~Dev() {
    for (int k = 0; k < np; k++) (void)hipFree(p[k]);
  }
};

template <typename Kern>
int gp_run_comp(Kern kern, uint32_t n_in, uint32_t lanes, const uint8_t* active, const uint32_t* in, uint32_t* out) {
  if (!gp::comp_args_ok(lanes, active, in, out)) return (int)hipErrorInvalidValue;
  const size_t out_b = (size_t)lanes * GP_COMP_OUT * 4;
  Dev d;
  const uint8_t* d_act = d.up(active, lanes / 2);
  const uint32_t* d_in = d.up(in, (size_t)(lanes / 2) * n_in * 4);
  uint32_t* d_out = d.up(out, out_b);   // arrives pre-filled (poison): inactive rows come back as they went in
  if (d.e == hipSuccess) {
    hipLaunchKernelGGL(kern, dim3((lanes + 63) / 64), dim3(64), 0, 0, lanes, d_act, d_in, d_out);
    if (d.ran()) d.down(out, d_out, out_b);
  }
  return (int)d.e;
}
}  // namespace

extern "C" {
// every entry returns the HIP status (hipErrorInvalidValue for arguments the
// bounds forbid)
int gp_grp_mul_comp(uint32_t lanes, const uint8_t* active, const uint32_t* in, uint32_t* out) {
  return gp_run_comp(k_gp_mul_comp, GP_MUL_IN, lanes, active, in, out);
}
int gp_grp_sqr_comp(uint32_t lanes, const uint8_t* active, const uint32_t* in, uint32_t* out) {
  return gp_run_comp(k_gp_sqr_comp, GP_SQR_IN, lanes, active, in, out);
}

// heads: n words; ents: n x 32 x 4 words; img: n x n_slots x 24 words, read and written
int gp_round(uint32_t n, uint32_t n_slots, const uint8_t* active, const uint32_t* heads, const uint32_t* ents, uint32_t* img) {
  if (!gp::round_args_ok(n, n_slots, active, heads, ents, img)) return (int)hipErrorInvalidValue;
  const size_t img_b = (size_t)n * n_slots * 96;
  Dev d;
  const uint8_t* d_act = d.up(active, n);
  const uint32_t* d_heads = d.up(heads, (size_t)n * 4);
  const uint32_t* d_ents = d.up(ents, (size_t)n * GP_ROUND_ENTS * 16);
  uint32_t* d_img = d.up(img, img_b);
  if (d.e == hipSuccess) {
    hipLaunchKernelGGL(k_gp_round, dim3(n), dim3(64), 0, 0, n, d_act, n_slots, d_heads, reinterpret_cast<const uint4*>(d_ents),
                       reinterpret_cast<uint4*>(d_img));
    if (d.ran()) d.down(img, d_img, img_b);
  }
  return (int)d.e;
}

// fin: 144 m words (36 uint4 rows of m lanes); code_out: m bytes and gt_out:
// 576 m bytes, both arriving pre-filled
int gp_group_fe(uint32_t m, const uint32_t* fin, uint8_t* code_out, uint8_t* gt_out) {
  if (m == 0 || m > GP_MAX_ROWS || !fin || !code_out || !gt_out) return (int)hipErrorInvalidValue;
  Dev d;
  const uint32_t* d_fin = d.up(fin, (size_t)m * 576);
  uint8_t* d_code = d.up(code_out, m);
  uint8_t* d_gt = d.up(gt_out, (size_t)m * 576);
  if (d.e == hipSuccess) {
    hipLaunchKernelGGL(k_group_fe, dim3(m), dim3(64), 0, 0, m, reinterpret_cast<const uint4*>(d_fin), d_code, d_gt);
    if (d.ran()) {
      d.down(code_out, d_code, m);
      d.down(gt_out, d_gt, (size_t)m * 576);
    }
  }
  return (int)d.e;
}

// code, inf: n bytes; code2, inf2: n bytes or null; sig_aff, h_aff: 24 stride
// words; pk_aff: 48 stride words; alias != 0: the kernel's code_out is `code`
// itself (code_out then receives a copy of it); gt_out: 576 n bytes pre-filled
int gp_group(uint32_t n, uint32_t stride, const uint8_t* code, const uint8_t* inf, const uint8_t* code2, const uint8_t* inf2,
             const uint32_t* sig_aff, const uint32_t* h_aff, const uint32_t* pk_aff, int alias, uint8_t* code_out,
             uint8_t* gt_out) {
  if (n == 0 || n > GP_MAX_ROWS || stride < n || stride > 2 * GP_MAX_ROWS || !code || !inf || !sig_aff || !h_aff || !pk_aff ||
      !code_out || !gt_out)
    return (int)hipErrorInvalidValue;
  Dev d;
  uint8_t* d_code = d.up(code, n);
  const uint8_t* d_inf = d.up(inf, n);
  const uint8_t* d_code2 = d.up(code2, n);
  const uint8_t* d_inf2 = d.up(inf2, n);
  const uint32_t* d_sig = d.up(sig_aff, (size_t)stride * 96);
  const uint32_t* d_h = d.up(h_aff, (size_t)stride * 96);
  const uint32_t* d_pk = d.up(pk_aff, (size_t)stride * 192);
  uint8_t* d_out = alias ? d_code : d.up(code_out, n);
  uint8_t* d_gt = d.up(gt_out, (size_t)n * 576);
  if (d.e == hipSuccess) {
    hipLaunchKernelGGL(k_group, dim3(n), dim3(64), 0, 0, (uint64_t)n, d_code, d_inf, d_code2, d_inf2, d_sig, d_h, d_pk,
                       (uint64_t)stride, d_out, d_gt);
    if (d.ran()) {
      d.down(code_out, d_out, n);
      d.down(gt_out, d_gt, (size_t)n * 576);
    }
  }
  return (int)d.e;
}

// "name:words in:words out,..." of every entry point of the library
const char* group_probe_ops() { return GP_OPS_STRING; }
int group_probe_threads() { return 64; }
int group_probe_slots() { return grp::N_SLOTS; }
const char* group_probe_error(int status) { return hipGetErrorString((hipError_t)status); }
}
#endif
