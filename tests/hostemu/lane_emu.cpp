// TEST HARNESS ONLY: the lane functions of tests/probe/lane_probe.hip (the
// one-lane BLS headers, each primitive alone) compiled for the host
// (CESS_HOSTEMU) and run in a loop over the lanes, for
// tests/test_lane_primitives.py.  With -DLANE_EMU_MAIN a stand-alone program
// (its own main) that the sanitizer test runs as a child process.  Never
// linked into the product library.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

// soa.hpp's uint4 rows on the host
struct uint4 {
  uint32_t x, y, z, w;
};
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return {x, y, z, w}; }

#include "../probe/lane_probe.hip"

extern "C" {
// one operation of the probe on n lanes: 0, 1 for arguments the lanes' bounds
// forbid, 2 for an unknown name.  Inactive lanes keep what `out` held.
int emu_lp(const char* name, uint32_t n, const uint8_t* active, const uint32_t* in, uint32_t* out) {
#define X(op, NI, NO, CHK)                                                      \
  if (!strcmp(name, #op)) {                                                     \
    if (!lp::args_ok(NI, CHK, n, active, in, out)) return 1;                    \
    for (uint32_t i = 0; i < n; i++)                                            \
      if (active[i]) lp::l_##op(in + (uint64_t)i * NI, out + (uint64_t)i * NO); \
    return 0;                                                                   \
  }
  LP_OPS_ALL(X)
#undef X
  return 2;
}
// soa_layout, the entry with a buffer shared by all lanes (as lp_soa_layout)
int emu_lp_soa_layout(uint32_t n, uint32_t stride, const uint8_t* active, const uint32_t* in, uint32_t* slots,
                      const uint32_t* tab, uint32_t* out) {
  if (!lp::soa_args_ok(n, stride, active, in, slots, tab, out)) return 1;
  for (uint32_t i = 0; i < n; i++)
    if (active[i]) lp::l_soa_layout(i, stride, in + (uint64_t)i * LP_SOA_IN, slots, tab, out + (uint64_t)i * LP_SOA_OUT);
  return 0;
}
// "name:words in:words out,..."
const char* emu_lp_ops() {
  return ""
#define X(op, NI, NO, CHK) #op ":" #NI ":" #NO ","
      LP_OPS_ALL(X)
#undef X
      "soa_layout:72:252,";
}
}  // extern "C"

#if defined(LANE_EMU_MAIN)
// ops file: per operation "name n n_in n_out", then n * n_in words, all
// decimal; the results go to the output file, n * n_out words per operation,
// every lane active
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "r");
  FILE* o = fopen(argv[2], "w");
  if (!f || !o) return 2;
  char name[64];
  unsigned n, n_in, n_out;
  int ops = 0;
  while (fscanf(f, "%63s %u %u %u", name, &n, &n_in, &n_out) == 4) {
    if (!strcmp(name, "soa_layout")) {   // then the stride, the rows, the table; results: out, then the slots
      unsigned stride;
      if (n_in != LP_SOA_IN || n_out != LP_SOA_OUT || fscanf(f, "%u", &stride) != 1 || stride < n || stride > (1u << 17)) return 2;
      std::vector<uint32_t> in((size_t)n * n_in), out((size_t)n * n_out, 0xDEADBEEFu), tab(LP_SOA_TAB);
      std::vector<uint32_t> slots((size_t)LP_SOA_SLOT_ROWS * stride, 0xA5A5A5A5u);
      std::vector<uint8_t> active(n, 1);
      for (auto& w : in)
        if (fscanf(f, "%u", &w) != 1) return 2;
      for (auto& w : tab)
        if (fscanf(f, "%u", &w) != 1) return 2;
      if (emu_lp_soa_layout(n, stride, active.data(), in.data(), slots.data(), tab.data(), out.data())) return 1;
      for (size_t i = 0; i < out.size(); i++) fprintf(o, "%u\n", out[i]);
      for (size_t i = 0; i < slots.size(); i++) fprintf(o, "%u\n", slots[i]);
      ops++;
      continue;
    }
    bool match = false;   // the file's layout must be the entry's own
#define X(op, NI, NO, CHK) \
  if (!strcmp(name, #op)) match = n_in == NI && n_out == NO;
    LP_OPS_ALL(X)
#undef X
    if (!match) {
      printf("%s: unknown operation or layout\n", name);
      return 2;
    }
    std::vector<uint32_t> in((size_t)n * n_in), out((size_t)n * n_out, 0xDEADBEEFu);
    std::vector<uint8_t> active(n, 1);
    for (auto& w : in)
      if (fscanf(f, "%u", &w) != 1) return 2;
    const int rc = emu_lp(name, n, active.data(), in.data(), out.data());
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
