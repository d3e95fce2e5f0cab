// Host build of cess_amd/csrc/ed25519.hpp (-DCESS_HOSTEMU) for
// tests/test_ed25519.py: the field, scalar and group code of the Ed25519
// kernels, and a per-record verify that follows k_ed25519_keys /
// k_ed25519_verify step by step (the hash is rsa_digest512.hpp's compression
// over a locally padded buffer).  With -DED25519_EMU_MAIN it is a stand-alone
// program over a text file of records, or (first argument "ops") over a file of
// primitive operand tables whose results it writes out (the sanitizer runs).
// emu_edp runs the lane functions of tests/probe/ed25519_probe.hip, the GPU
// probe's own, in a loop over the lanes (tests/test_ed25519_primitives.py).
// Never linked into the product library.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../cess_amd/csrc/ed25519.hpp"
#include "../../cess_amd/csrc/rsa_digest512.hpp"
#include "../probe/ed25519_probe.hip"   // the lane functions and EDP_OPS (no device code under CESS_HOSTEMU)

using namespace ed25519;

namespace {

void sha512(const std::vector<uint8_t>& m, uint8_t out[64]) {
  std::vector<uint8_t> p(m);
  p.push_back(0x80);
  while (p.size() % 128 != 112) p.push_back(0);
  for (int i = 0; i < 8; i++) p.push_back(0);
  const uint64_t bits = (uint64_t)m.size() * 8;
  for (int i = 7; i >= 0; i--) p.push_back((uint8_t)(bits >> (8 * i)));
  uint64_t st[8];
  for (int i = 0; i < 8; i++) st[i] = rsa_digest512::SHA512_IV[i];
  for (size_t b = 0; b < p.size(); b += 128) {
    uint32_t blk[32];
    for (int j = 0; j < 32; j++)
      blk[j] = ((uint32_t)p[b + 4 * j] << 24) | ((uint32_t)p[b + 4 * j + 1] << 16) | ((uint32_t)p[b + 4 * j + 2] << 8) |
               p[b + 4 * j + 3];
    rsa_digest512::sha512_compress(st, blk);
  }
  for (int j = 0; j < 64; j++) out[j] = (uint8_t)(st[j >> 3] >> (56 - 8 * (j & 7)));
}

fe fe_of(const uint32_t* a) {
  fe r;
  for (int i = 0; i < 10; i++) r.v[i] = a[i];
  return r;
}

uint32_t g_tab_b[kTableWords];
bool g_tab_b_ready = false;

// one record as the two kernels see it: the key's table and status, then the codes in order
int verify_one(const uint8_t* key, uint64_t key_len, const uint8_t* msg, uint64_t msg_len, const uint8_t* sig,
               uint64_t sig_len) {
  if (!g_tab_b_ready) {
    key_table(kNegBaseEnc, 32, g_tab_b);   // multiples of B
    g_tab_b_ready = true;
  }
  uint32_t tab_a[kTableWords];
  const uint8_t st = key_table(key, key_len, tab_a);
  uint32_t S[8] = {0}, R[8] = {0};
  if (sig_len == 64) {
    load_words(sig, R);
    load_words(sig + 32, S);
  }
  const uint32_t early = early_code(st, sig_len, S);
  std::vector<uint8_t> in;
  if (sig_len == 64) in.insert(in.end(), sig, sig + 32);
  else in.insert(in.end(), 32, 0);
  if (key_len == 32) in.insert(in.end(), key, key + 32);
  else in.insert(in.end(), 32, 0);
  in.insert(in.end(), msg, msg + msg_len);
  uint8_t dig[64];
  sha512(in, dig);
  uint32_t x[16], h[8];
  for (int i = 0; i < 16; i++)
    x[i] = (uint32_t)dig[4 * i] | ((uint32_t)dig[4 * i + 1] << 8) | ((uint32_t)dig[4 * i + 2] << 16) |
           ((uint32_t)dig[4 * i + 3] << 24);
  sc_reduce512(x, h);
  const bool active = early == ED_OK;
  if (!active)
    for (int i = 0; i < 8; i++) S[i] = h[i] = 0;
  const bool ok = verify_equation(active ? tab_a : g_tab_b, g_tab_b, S, h, R);
  return (int)(active ? (ok ? ED_OK : ED_MISMATCH) : early);
}

}  // namespace

extern "C" {

// op: 0 mul, 1 sqr, 2 add, 3 sub, 4 neg, 5 carry, 6 invert, 7 pow22523, 8 neg_tight
void emu_ed_fe_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  const fe x = fe_of(a), y = fe_of(b);
  fe r;
  switch (op) {
    case 0: r = fe_mul(x, y); break;
    case 1: r = fe_sqr(x); break;
    case 2: r = fe_add(x, y); break;
    case 3: r = fe_sub(x, y); break;
    case 4: r = fe_neg(x); break;
    case 5: r = fe_carry(x); break;
    case 6: r = fe_invert(x); break;
    case 7: r = fe_pow22523(x); break;
    default: r = fe_neg_tight(x); break;
  }
  for (int i = 0; i < 10; i++) out[i] = r.v[i];
}
void emu_ed_fe_frombytes(const uint8_t* b, uint32_t* out) {
  uint32_t w[8];
  load_words(b, w);
  const fe r = fe_from_words(w);
  for (int i = 0; i < 10; i++) out[i] = r.v[i];
}
// canonical 32 bytes; returns is_zero | is_negative << 1
int emu_ed_fe_tobytes(const uint32_t* a, uint8_t* out) {
  uint32_t w[8];
  const fe x = fe_of(a);
  fe_to_words(x, w);
  memcpy(out, w, 32);
  return (fe_is_zero(x) ? 1 : 0) | (int)(fe_is_negative(x) << 1);
}
// the 128-bit maximum of every column sum since the last reset
void emu_ed_col_max(uint64_t* hi, uint64_t* lo, int reset) {
  *hi = (uint64_t)(g_col_max >> 64);
  *lo = (uint64_t)g_col_max;
  if (reset) g_col_max = 0;
}
int emu_ed_sc_lt_l(const uint8_t* s) {
  uint32_t w[8];
  load_words(s, w);
  return sc_lt_L(w) ? 1 : 0;
}
void emu_ed_sc_reduce(const uint8_t* x64, uint8_t* out32) {
  uint32_t x[16], r[8];
  memcpy(x, x64, 64);
  sc_reduce512(x, r);
  memcpy(out32, r, 32);
}
// the 64 digits, most significant first, as the verify loop reads them
void emu_ed_sc_digits(const uint8_t* s, int8_t* digits) {
  uint32_t w[8], r[8];
  load_words(s, w);
  sc_recode(w, r);
  for (int i = 0; i < 64; i++) digits[i] = (int8_t)sc_top_digit(r);
}
int emu_ed_key_table(const uint8_t* key, uint64_t len, uint32_t* tab) { return key_table(key, len, tab); }
int emu_ed_verify(const uint8_t* key, uint64_t key_len, const uint8_t* msg, uint64_t msg_len, const uint8_t* sig,
                  uint64_t sig_len) {
  return verify_one(key, key_len, msg, msg_len, sig, sig_len);
}

// one operation of the probe on n lanes: 0, 1 for arguments the lanes' bounds
// forbid, 2 for an unknown name.  Inactive lanes keep what `out` held.
int emu_edp(const char* name, uint32_t n, const uint8_t* active, const uint32_t* in, uint32_t* out, const uint32_t* tabs,
            uint32_t n_tabs) {
#define X(op, NI, NO, NIDX, T)                                                    \
  if (!strcmp(name, #op)) {                                                       \
    if (!edp::args_ok(NI, NIDX, n, active, in, out, tabs, n_tabs)) return 1;      \
    for (uint32_t i = 0; i < n; i++)                                              \
      if (active[i]) edp::l_##op(in + (uint64_t)i * NI, out + (uint64_t)i * NO, tabs); \
    return 0;                                                                     \
  }
  EDP_OPS(X)
#undef X
  return 2;
}
// "name:words in:words out:table indices:threads,..."
const char* emu_edp_ops() {
  return ""
#define X(op, NI, NO, NIDX, T) #op ":" #NI ":" #NO ":" #NIDX ":" #T ","
      EDP_OPS(X)
#undef X
      ;
}

}  // extern "C"

#if defined(ED25519_EMU_MAIN)
// records file: one record per line, "keyhex msghex sighex code" with "-" for an empty field
static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return out;
}
// ops file: per operation "name n n_in n_out n_tabs", then n * n_in words and
// n_tabs * 240 words, all decimal; the results go to the output file, n * n_out
// words per operation, every lane active
static int run_ops(const char* in_path, const char* out_path) {
  FILE* f = fopen(in_path, "r");
  FILE* o = fopen(out_path, "w");
  if (!f || !o) return 2;
  char name[64];
  unsigned n, n_in, n_out, n_tabs;
  int ops = 0;
  while (fscanf(f, "%63s %u %u %u %u", name, &n, &n_in, &n_out, &n_tabs) == 5) {
    std::vector<uint32_t> in((size_t)n * n_in), out((size_t)n * n_out, 0xDEADBEEFu), tabs((size_t)n_tabs * kTableWords);
    std::vector<uint8_t> active(n, 1);
    for (auto& w : in)
      if (fscanf(f, "%u", &w) != 1) return 2;
    for (auto& w : tabs)
      if (fscanf(f, "%u", &w) != 1) return 2;
    const int rc = emu_edp(name, n, active.data(), in.data(), out.data(), n_tabs ? tabs.data() : nullptr, n_tabs);
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
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "ops")) return argc == 4 ? run_ops(argv[2], argv[3]) : 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char k[8192], m[8192], s[8192];
  int want, n = 0, bad = 0;
  while (fscanf(f, "%8191s %8191s %8191s %d", k, m, s, &want) == 4) {
    const std::vector<uint8_t> key = unhex(k), msg = unhex(m), sig = unhex(s);
    const int got = verify_one(key.data(), key.size(), msg.data(), msg.size(), sig.data(), sig.size());
    if (got != want) {
      printf("record %d: code %d, expected %d\n", n, got, want);
      bad++;
    }
    n++;
  }
  fclose(f);
  printf("%d records, %d wrong\n", n, bad);
  return bad ? 1 : 0;
}
#endif
