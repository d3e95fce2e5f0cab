// TEST HARNESS ONLY: the lane functions of tests/probe/group_probe.hip (the
// lane-group half-products grp_mul_comp / grp_sqr_comp of bls/group.hpp, each
// alone) and one round of a lane-group program over group_eval_comp, compiled
// for the host (CESS_HOSTEMU) for tests/test_group_primitives.py.  The round
// has the kernel's semantics: every lane of the round reads the register file
// before any lane writes it.  With -DGROUP_EMU_MAIN a stand-alone program (its
// own main) that the sanitizer test runs as a child process.  Never linked into
// the product library.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../probe/group_probe.hip"

namespace {
// a row's register-file image: 24 words per slot, c0 then c1
struct ImgRegs {
  const uint32_t* S;
  bls::fp2 ld(uint32_t s) const { return gp::ldf2(S + 24 * s); }
  bls::fp ld_comp(uint32_t s, uint32_t comp) const { return gp::ldf(S + 24 * s + 12 * comp); }
};
struct Write {
  uint32_t slot, comp;
  bls::fp v;
};
}  // namespace

extern "C" {
// 0, or 1 for arguments the bounds forbid.  Inactive rows keep what `out` held.
int emu_gp_grp_mul_comp(uint32_t lanes, const uint8_t* active, const uint32_t* in, uint32_t* out) {
  if (!gp::comp_args_ok(lanes, active, in, out)) return 1;
  for (uint32_t i = 0; i < lanes; i++)
    if (active[i >> 1]) gp::l_grp_mul_comp(in + (uint64_t)(i >> 1) * GP_MUL_IN, out + (uint64_t)i * GP_COMP_OUT, i & 1u);
  return 0;
}
int emu_gp_grp_sqr_comp(uint32_t lanes, const uint8_t* active, const uint32_t* in, uint32_t* out) {
  if (!gp::comp_args_ok(lanes, active, in, out)) return 1;
  for (uint32_t i = 0; i < lanes; i++)
    if (active[i >> 1]) gp::l_grp_sqr_comp(in + (uint64_t)(i >> 1) * GP_SQR_IN, out + (uint64_t)i * GP_COMP_OUT, i & 1u);
  return 0;
}
// one round per row on the row's image (as gp_round): the kernel's lanes, lane
// 2 op + comp computing component comp of op; all reads, then all writes
int emu_gp_round(uint32_t n, uint32_t n_slots, const uint8_t* active, const uint32_t* heads, const uint32_t* ents, uint32_t* img) {
  if (!gp::round_args_ok(n, n_slots, active, heads, ents, img)) return 1;
  std::vector<Write> wr;
  for (uint32_t i = 0; i < n; i++) {
    if (!active[i]) continue;
    uint32_t* S = img + (uint64_t)i * 24 * n_slots;
    const ImgRegs R{S};
    const uint32_t h = heads[i], kind = h & 0xffu, cnt = (h >> 8) & 0xffu, off = h >> 16;
    wr.clear();
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint32_t op = lane >> 1, comp = lane & 1;
      if (op >= cnt) continue;
      const uint32_t* e = ents + ((uint64_t)i * GP_ROUND_ENTS + off + op) * 4;
      uint32_t d;
      const bls::fp v = bls::group_eval_comp(R, kind, e[0], e[1], e[2], e[3], comp, &d);
      wr.push_back({d, comp, v});
    }
    for (const Write& w : wr) gp::stf(S + 24 * w.slot + 12 * w.comp, w.v);
  }
  return 0;
}
const char* emu_gp_ops() { return GP_OPS_STRING; }
int emu_gp_slots() { return grp::N_SLOTS; }
int emu_gp_consts() { return grp::N_CONSTS; }
}  // extern "C"

#if defined(GROUP_EMU_MAIN)
// ops file, all decimal: "grp_mul_comp lanes" or "grp_sqr_comp lanes", then the
// rows' words; "round n n_slots", then n heads, n x 128 entry words and the
// images.  The results go to the output file (the lanes' words; the images),
// every row active.
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "r");
  FILE* o = fopen(argv[2], "w");
  if (!f || !o) return 2;
  char name[64];
  unsigned n;
  int ops = 0;
  auto read = [&](std::vector<uint32_t>& v) {
    for (auto& w : v)
      if (fscanf(f, "%u", &w) != 1) return false;
    return true;
  };
  while (fscanf(f, "%63s %u", name, &n) == 2) {
    if (n == 0 || n > 2 * GP_MAX_ROWS) return 2;
    int rc;
    std::vector<uint32_t> out;
    if (!strcmp(name, "round")) {
      unsigned n_slots;
      if (fscanf(f, "%u", &n_slots) != 1 || n_slots == 0 || n_slots > (unsigned)grp::N_SLOTS) return 2;
      std::vector<uint32_t> heads(n), ents((size_t)n * 4 * GP_ROUND_ENTS);
      out.resize((size_t)n * 24 * n_slots);
      std::vector<uint8_t> active(n, 1);
      if (!read(heads) || !read(ents) || !read(out)) return 2;
      rc = emu_gp_round(n, n_slots, active.data(), heads.data(), ents.data(), out.data());
    } else {
      const bool mul = !strcmp(name, "grp_mul_comp");
      if (!mul && strcmp(name, "grp_sqr_comp")) {
        printf("%s: unknown operation\n", name);
        return 2;
      }
      std::vector<uint32_t> in((size_t)(n / 2) * (mul ? GP_MUL_IN : GP_SQR_IN));
      out.assign((size_t)n * GP_COMP_OUT, 0xDEADBEEFu);
      std::vector<uint8_t> active(n / 2 + 1, 1);
      if (!read(in)) return 2;
      rc = mul ? emu_gp_grp_mul_comp(n, active.data(), in.data(), out.data())
               : emu_gp_grp_sqr_comp(n, active.data(), in.data(), out.data());
    }
    if (rc) {
      printf("%s: status %d\n", name, rc);
      return 1;
    }
    for (size_t i = 0; i < out.size(); i++) fprintf(o, "%u\n", out[i]);
    ops++;
  }
  fclose(f);
  fclose(o);
  printf("%d operations\n", ops);
  return 0;
}
#endif
