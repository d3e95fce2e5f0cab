// Host build of cess_amd/csrc/p256.hpp (-DCESS_HOSTEMU) for tests/test_ecdsa.py
// and tests/test_ecdsa_primitives.py: emu_ecp runs the lane functions of
// tests/probe/ecdsa_probe.hip, the GPU probe's own, in a loop over the lanes,
// and emu_ecdsa_record follows k_ecdsa_keys / k_ecdsa_pack / k_ecdsa_verify
// step by step on one record (the digest comes from the caller: the digest
// kernels have their own tests).  With -DECDSA_EMU_MAIN it is a stand-alone
// program over a text file of records "alg key sig digest code" (hex, "-" for
// empty, key "x" for an index outside the table) and a file of primitive rows
// "op words-in..." whose results it writes out (the sanitizer runs).  Never
// linked into the product library.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../probe/ecdsa_probe.hip"   // the lane functions and ECP_OPS (no device code under CESS_HOSTEMU)

using namespace p256;

namespace {

uint32_t g_tab_g[kTableWords];
bool g_tab_g_ready = false;

struct Op {
  const char* name;
  uint32_t ni, no, nidx, len_at, len_max;
  void (*fn)(const uint32_t*, uint32_t*, const uint32_t*);
};
const Op kOps[] = {
#define X(name, NI, NO, NIDX, T, LA, LM) {#name, NI, NO, NIDX, LA, LM, ecp::l_##name},
    ECP_OPS(X)
#undef X
};
const Op* find_op(const char* name) {
  for (const Op& o : kOps)
    if (strcmp(o.name, name) == 0) return &o;
  return nullptr;
}

}  // namespace

extern "C" {

// the lane function `name` over n lanes; -1: no such entry, -2: arguments the lanes' bounds forbid
int emu_ecp(const char* name, uint32_t n, const uint8_t* active, const uint32_t* in, uint32_t* out, const uint32_t* tabs,
            uint32_t n_tabs) {
  const Op* o = find_op(name);
  if (!o) return -1;
  if (!ecp::args_ok(o->ni, o->nidx, o->len_at, o->len_max, n, active, in, out, tabs, n_tabs)) return -2;
  for (uint32_t i = 0; i < n; i++)
    if (active[i]) o->fn(in + (uint64_t)i * o->ni, out + (uint64_t)i * o->no, tabs);
  return 0;
}

// one record as the three kernels see it; key = NULL: an index outside the table
int emu_ecdsa_record(uint32_t alg, const uint8_t* key, uint64_t key_len, const uint8_t* sig, uint64_t sig_len,
                     const uint8_t* digest) {
  if (!g_tab_g_ready) {
    key_table(kGEnc, 65, g_tab_g);
    g_tab_g_ready = true;
  }
  uint32_t tab_q[kTableWords];
  const bool key_ok = key && key_table(key, key_len, tab_q) == KEY_LOADED;
  uint32_t r[8], s[8], e[8];
  const uint32_t code = parse_sig(alg, sig, sig_len, r, s);
  const uint32_t early = key_ok ? code : (uint32_t)EC_KEY;
  if (early != EC_OK) return (int)early;
  digest_scalar(digest, e);
  return verify_scalars(tab_q, g_tab_g, e, r, s) ? (int)EC_OK : (int)EC_MISMATCH;
}

// the largest column sum seen since the last reset, as two 64-bit halves
void emu_ecdsa_col_max(uint64_t* lo, uint64_t* hi, int reset) {
  *lo = (uint64_t)g_col_max;
  *hi = (uint64_t)(g_col_max >> 64);
  if (reset) g_col_max = 0;
}
uint64_t emu_ecdsa_col_bound() { return kColBound; }

// how often pt_madd took each special return since the last reset: an infinite
// first operand, a doubling, a cancel to infinity (key_table's first addition
// is a doubling: one per table built)
void emu_ecdsa_madd_counts(uint64_t* out3, int reset) {
  for (int i = 0; i < 3; i++) out3[i] = g_madd_seen[i];
  if (reset)
    for (int i = 0; i < 3; i++) g_madd_seen[i] = 0;
}

}  // extern "C"

#if defined(ECDSA_EMU_MAIN)
namespace {
bool unhex(const std::string& h, std::vector<uint8_t>& out) {
  out.clear();
  if (h == "-") return true;
  if (h.size() % 2) return false;
  for (size_t i = 0; i < h.size(); i += 2) {
    unsigned v;
    if (sscanf(h.c_str() + i, "%2x", &v) != 1) return false;
    out.push_back((uint8_t)v);
  }
  return true;
}
}  // namespace

// ecdsa_emu records.txt ops.txt ops_out.txt
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  char a[16], k[600], s[600], d[200];
  int want, total = 0, wrong = 0;
  while (fscanf(f, "%15s %599s %599s %199s %d", a, k, s, d, &want) == 5) {
    std::vector<uint8_t> key, sig, dig;
    const bool no_key = strcmp(k, "x") == 0;
    if ((!no_key && !unhex(k, key)) || !unhex(s, sig) || !unhex(d, dig) || dig.size() < 32) return 2;
    key.push_back(0), sig.push_back(0);   // (a non-null pointer for the empty ones)
    const int got = emu_ecdsa_record((uint32_t)atoi(a), no_key ? nullptr : key.data(), key.size() - 1, sig.data(),
                                     sig.size() - 1, dig.data());
    total++;
    if (got != want) wrong++, printf("record %d: got %d want %d\n", total, got, want);
  }
  fclose(f);
  printf("%d records, %d wrong\n", total, wrong);
  printf("madd returns: %llu infinite, %llu doubling, %llu cancel\n", (unsigned long long)g_madd_seen[MADD_INF],
         (unsigned long long)g_madd_seen[MADD_DBL], (unsigned long long)g_madd_seen[MADD_CANCEL]);
  // the primitive rows: "op w0 w1 ..." -> "op o0 o1 ..."
  f = fopen(argv[2], "r");
  FILE* o = fopen(argv[3], "w");
  if (!f || !o) return 2;
  uint32_t tabs[2 * kTableWords];
  key_table(kGEnc, 65, tabs);
  key_table(kGEnc, 65, tabs + kTableWords);
  char name[64];
  int rows = 0;
  while (fscanf(f, "%63s", name) == 1) {
    const Op* op = find_op(name);
    if (!op) return 2;
    std::vector<uint32_t> in(op->ni), out(op->no, 0xa5a5a5a5u);
    for (uint32_t i = 0; i < op->ni; i++)
      if (fscanf(f, "%x", &in[i]) != 1) return 2;
    const uint8_t act = 1;
    if (emu_ecp(name, 1, &act, in.data(), out.data(), tabs, 2) != 0) return 2;
    fprintf(o, "%s", name);
    for (uint32_t v : out) fprintf(o, " %x", v);
    fprintf(o, "\n");
    rows++;
  }
  fclose(f);
  fclose(o);
  printf("%d primitive rows\n", rows);
  return wrong ? 1 : 0;
}
#endif
