// Host build of the RSA kernels' arithmetic (cess_amd/csrc/k_rsa.hpp: the
// expanded 1024 / 2048-bit classes; rsa_mont.hpp: the loop-form class) for
// tests/test_rsa_primitives.py: every
// Montgomery primitive alone, the one-record verifier of each class, and the
// largest column value the 128-bit shadow of the 64-bit accumulators saw.  The
// loop-form kernel comes from rsa_big_emu.cpp (k_rsa_big.hip built for the
// host), which is compiled and linked together with this file.
// With -DRSA_EMU_MAIN the same entries run from a stand-alone program (for a
// build under the address and undefined-behaviour sanitizers): it reads the
// test's row file and writes the results for the test to check.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cess_amd/csrc/k_rsa.hpp"
#include "../../cess_amd/csrc/rsa_mont.hpp"

enum { OP_MUL = 0, OP_SQR = 1, OP_CANON = 2, OP_WORDS = 3, OP_MONT_RT = 4, OP_VERIFY = 5 };

// out aliases a, as in every production call of mont<L, SQR>
template <int L>
static void rows_fixed(int op, int rows, const uint32_t* n, const uint32_t* ninv, const uint32_t* a, const uint32_t* b,
                       uint32_t* out) {
  constexpr int W = (28 * L + 31) / 32;
  for (int r = 0; r < rows; r++) {
    uint32_t nn[L], x[L], y[L];
    for (int i = 0; i < L; i++) nn[i] = n[(size_t)r * L + i], x[i] = a[(size_t)r * L + i], y[i] = b[(size_t)r * L + i];
    if (op == OP_WORDS) {
      uint32_t w[W];
      rsa_detail::to_words<L, W>(x, w);
      for (int j = 0; j < W; j++) out[(size_t)r * W + j] = w[j];
      continue;
    }
    if (op == OP_MUL) rsa_detail::mont<L, false>(x, y, nn, ninv[r], x);
    if (op == OP_SQR) rsa_detail::mont<L, true>(x, x, nn, ninv[r], x);
    if (op == OP_CANON) rsa_detail::canon<L>(x, nn);
    for (int i = 0; i < L; i++) out[(size_t)r * L + i] = x[i];
  }
}

// results per row: L words (OP_WORDS: (28 L + 31) / 32; OP_MONT_RT: L + 1).
// Returns 0, or -1 for an operation / limb count this build does not have.
extern "C" int emu_rsa_rows(int op, int L, int rows, const uint32_t* n, const uint32_t* ninv, const uint32_t* a,
                            const uint32_t* b, uint32_t* out) {
  if (op == OP_MONT_RT) {
    if (L <= 0 || L > RSA_LMAX || L % RSA_BIG_ROWS) return -1;
    for (int r = 0; r < rows; r++)
      rsa_big::mont_rt(a + (size_t)r * L, b + (size_t)r * L, n + (size_t)r * L, ninv[r], L, out + (size_t)r * (L + 1));
    return 0;
  }
  if (op < OP_MUL || op > OP_WORDS) return -1;
  if (L == RSA_L1024) rows_fixed<RSA_L1024>(op, rows, n, ninv, a, b, out);
  else if (L == RSA_L2048) rows_fixed<RSA_L2048>(op, rows, n, ninv, a, b, out);
  else return -1;
  return 0;
}

// k_rsa_verify_big's body on one record (rsa_big_emu.cpp)
extern "C" int emu_rsa_verify_big(int L, uint32_t k_bytes, uint64_t e, const uint32_t* n28, const uint32_t* r2_28,
                                  uint32_t ninv, const uint8_t* sig, const uint8_t* msg, uint32_t msg_len);

// one record through the class's verifier (t = 0, cnt = 1; the key row as
// the host would build it, computed by the caller): the code, 0xff if none
// was written
extern "C" int emu_rsa_verify(int L, uint32_t k_bytes, uint64_t e, const uint32_t* n28, const uint32_t* r2_28,
                              uint32_t ninv, const uint8_t* sig, const uint8_t* msg, uint32_t msg_len) {
  if (L <= 0 || L > RSA_LMAX) return -1;
  if (L != RSA_L1024 && L != RSA_L2048) return emu_rsa_verify_big(L, k_bytes, e, n28, r2_28, ninv, sig, msg, msg_len);
  std::vector<RsaKeyDev> keys(1);
  RsaKeyDev& K = keys[0];
  memset(&K, 0, sizeof(K));
  K.k_bytes = k_bytes, K.ninv = ninv, K.limbs = (uint32_t)L, K.e = e;
  for (int i = 0; i < L; i++) K.n28[i] = n28[i], K.r2_28[i] = r2_28[i];
  const uint32_t rec[1] = {0}, key_idx[1] = {0};
  const uint64_t sig_offs[2] = {0, k_bytes}, msg_offs[2] = {0, msg_len};
  // exact-size copies, so that a read past either end is a sanitizer finding
  std::vector<uint8_t> s(sig, sig + k_bytes), m(msg, msg + msg_len);
  std::vector<uint32_t> base(L);
  uint8_t codes[1] = {0xff};
  if (L == RSA_L1024)
    rsa_verify_lane<RSA_L1024>(0, 1, rec, key_idx, keys.data(), s.data(), sig_offs, m.data(), msg_offs, base.data(), codes);
  else
    rsa_verify_lane<RSA_L2048>(0, 1, rec, key_idx, keys.data(), s.data(), sig_offs, m.data(), msg_offs, base.data(), codes);
  return codes[0];
}

// the largest column value seen (which = 0: mont<L, SQR> of k_rsa.hpp; 1: the
// u values of mont_rt) as two 64-bit halves; reset != 0 clears it afterwards
extern "C" void emu_rsa_col_max(int which, uint64_t* hi, uint64_t* lo, int reset) {
  unsigned __int128& m = which ? rsa_big::g_col_max : rsa_detail::g_col_max;
  *hi = (uint64_t)(m >> 64);
  *lo = (uint64_t)m;
  if (reset) m = 0;
}

#if defined(RSA_EMU_MAIN)
// rsa_emu IN OUT: IN is a sequence of sections, each a header of four uint32
// (op, L, rows, 0) and then, for the row operations, n (rows x L), ninv (rows),
// a and b (rows x L each); for OP_VERIFY, per row: k_bytes, e low, e high,
// ninv, msg_len, n (L), R^2 mod n (L), the signature and the message, each
// padded to whole words.  OUT takes the results in the same order (OP_VERIFY:
// one word per row) and, last, the two column maxima as four words each
// (most significant first).
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> in;
  uint32_t buf[4096];
  for (size_t got; (got = fread(buf, 4, 4096, f)) > 0;) in.insert(in.end(), buf, buf + got);
  fclose(f);
  std::vector<uint32_t> res;
  size_t p = 0, sections = 0, total = 0;
  auto need = [&](size_t words) {
    if (p + words > in.size()) {
      fprintf(stderr, "truncated input\n");
      exit(2);
    }
  };
  while (p < in.size()) {
    need(4);
    const int op = (int)in[p], L = (int)in[p + 1], rows = (int)in[p + 2];
    p += 4;
    if (L <= 0 || L > RSA_LMAX || rows < 0) return 2;
    if (op == OP_VERIFY) {
      for (int r = 0; r < rows; r++) {
        need(5);
        const uint32_t kb = in[p], ninv = in[p + 3], ml = in[p + 4];
        const uint64_t e = (uint64_t)in[p + 1] | (uint64_t)in[p + 2] << 32;
        p += 5;
        const size_t sw = (kb + 3) / 4, mw = (ml + 3) / 4;
        need(2 * (size_t)L + sw + mw);
        const uint32_t *n = &in[p], *r2 = &in[p + L];
        std::vector<uint8_t> sig(4 * sw + 1), msg(4 * mw + 1);
        memcpy(sig.data(), in.data() + p + 2 * L, 4 * sw);
        memcpy(msg.data(), in.data() + p + 2 * L + sw, 4 * mw);
        p += 2 * (size_t)L + sw + mw;
        res.push_back((uint32_t)emu_rsa_verify(L, kb, e, n, r2, ninv, sig.data(), msg.data(), ml));
      }
    } else {
      const size_t rl = (size_t)rows * L;
      need(3 * rl + rows);
      const size_t per = op == OP_WORDS ? (28 * (size_t)L + 31) / 32 : op == OP_MONT_RT ? L + 1 : L;
      // exact-size arrays, so that a read or write past an end is a sanitizer finding
      const uint32_t* s = in.data() + p;
      const std::vector<uint32_t> n(s, s + rl), ninv(s + rl, s + rl + rows), a(s + rl + rows, s + 2 * rl + rows),
          b(s + 2 * rl + rows, s + 3 * rl + rows);
      std::vector<uint32_t> out(per * rows);
      if (emu_rsa_rows(op, L, rows, n.data(), ninv.data(), a.data(), b.data(), out.data())) return 2;
      res.insert(res.end(), out.begin(), out.end());
      p += 3 * rl + rows;
    }
    sections++, total += rows;
  }
  for (int which = 0; which < 2; which++) {
    uint64_t hi, lo;
    emu_rsa_col_max(which, &hi, &lo, 0);
    res.push_back((uint32_t)(hi >> 32)), res.push_back((uint32_t)hi);
    res.push_back((uint32_t)(lo >> 32)), res.push_back((uint32_t)lo);
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(res.data(), 4, res.size(), f) != res.size() || fclose(f)) return 2;
  printf("%zu sections, %zu rows\n", sections, total);
  return 0;
}
#endif
