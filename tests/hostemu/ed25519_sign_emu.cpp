// Host build of cess_amd/csrc/ed25519_sign.hpp (-DCESS_HOSTEMU) for
// tests/test_ed25519_sign.py: the signer's scalar and group code, the comb
// table, and a per-signer / per-record path that follows k_ed25519_comb,
// k_ed25519_signers, k_ed25519_sign_r and k_ed25519_sign_s step by step (the
// hash is rsa_digest512.hpp's compression over a locally padded buffer).  With
// -DED25519_SIGN_EMU_MAIN it is a stand-alone program over a text file of
// records (the sanitizer run).  emu_edsp runs the lane functions of
// tests/probe/ed25519_sign_probe.hip, the GPU probe's own, in a loop over the
// lanes.  Never linked into the product library.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../cess_amd/csrc/ed25519_sign.hpp"
#include "../../cess_amd/csrc/rsa_digest512.hpp"
#include "../probe/ed25519_sign_probe.hip"   // the lane functions and EDSP_OPS (no device code under CESS_HOSTEMU)

using namespace ed25519;

namespace {

void sha512(const std::vector<uint8_t>& m, uint32_t (&x)[16]) {
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
  alignas(4) uint8_t out[64];
  for (int j = 0; j < 64; j++) out[j] = (uint8_t)(st[j >> 3] >> (56 - 8 * (j & 7)));
  load_digest(out, x);
}

uint32_t g_comb[kCombWords];
bool g_comb_ready = false;

const uint32_t* comb() {
  if (!g_comb_ready) {
    for (int i = 0; i < kCombRows; i++)
      if (comb_row(i, g_comb + kTableWords * i) != KEY_LOADED) abort();
    g_comb_ready = true;
  }
  return g_comb;
}

// one signer as k_ed25519_signers sees it
struct Signer {
  uint32_t a[8], prefix[8], A[8];
  uint8_t status;
};
Signer derive(const uint8_t* seed, uint64_t seed_len, const uint8_t* expected) {
  Signer s;
  uint32_t h[16];
  sha512(std::vector<uint8_t>(seed, seed + seed_len), h);
  s.status = signer_derive(comb(), h, seed_len == 32, expected, s.a, s.A);
  for (int q = 0; q < 8; q++) {
    s.a[q] = s.status == SIGNER_LOADED ? s.a[q] : 0u;
    s.prefix[q] = s.status == SIGNER_LOADED ? h[8 + q] : 0u;
    s.A[q] = seed_len == 32 ? s.A[q] : 0u;
  }
  return s;
}

// one record as k_ed25519_sign_pack, k_ed25519_sign_r and k_ed25519_sign_s see it
int sign_one(const Signer& s, const uint8_t* msg, uint64_t msg_len, uint8_t* sig) {
  const bool ok = s.status == SIGNER_LOADED;
  uint8_t head[32];
  std::vector<uint8_t> in;
  uint32_t x[16], r[8], R[8], k[8], S[8];
  store_bytes32(head, s.prefix);
  in.insert(in.end(), head, head + 32);
  in.insert(in.end(), msg, msg + msg_len);
  sha512(in, x);
  sc_reduce512(x, r);
  for (int q = 0; q < 8; q++) r[q] = ok ? r[q] : 0u;
  ge_scalarmult_base(comb(), r, R);
  for (int q = 0; q < 8; q++) R[q] = ok ? R[q] : 0u;
  store_bytes32(sig, R);
  in.assign(sig, sig + 32);
  store_bytes32(head, s.A);
  if (!ok) memset(head, 0, 32);
  in.insert(in.end(), head, head + 32);
  in.insert(in.end(), msg, msg + msg_len);
  sha512(in, x);
  sc_reduce512(x, k);
  sc_muladd(k, s.a, r, S);
  for (int q = 0; q < 8; q++) S[q] = ok ? S[q] : 0u;
  store_bytes32(sig + 32, S);
  return (int)(ok ? SIGN_OK : SIGN_SIGNER);
}

}  // namespace

extern "C" {

// the comb table: 64 rows of 240 words
void emu_eds_comb(uint32_t* out) { memcpy(out, comb(), sizeof g_comb); }
// the signer's status (SIGNER_*); pub_out: A, zeros for a seed that is not 32
// bytes; a_out (may be null): the stored scalar, a mod L
int emu_eds_signer(const uint8_t* seed, uint64_t seed_len, const uint8_t* expected, uint8_t* pub_out, uint8_t* a_out) {
  const Signer s = derive(seed, seed_len, expected);
  store_bytes32(pub_out, s.A);
  if (a_out) store_bytes32(a_out, s.a);
  return s.status;
}
// the record's code; sig_out: 64 bytes
int emu_eds_sign(const uint8_t* seed, uint64_t seed_len, const uint8_t* msg, uint64_t msg_len, uint8_t* sig_out) {
  return sign_one(derive(seed, seed_len, nullptr), msg, msg_len, sig_out);
}
// the 128-bit maximum of every column sum since the last reset
void emu_eds_col_max(uint64_t* hi, uint64_t* lo, int reset) {
  *hi = (uint64_t)(g_col_max >> 64);
  *lo = (uint64_t)g_col_max;
  if (reset) g_col_max = 0;
}
// one operation of the probe on n lanes: 0, 1 for arguments the lanes' bounds forbid, 2 for an unknown name
int emu_edsp(const char* name, uint32_t n, const uint32_t* in, uint32_t* out) {
#define X(op, NI, NO)                                                                             \
  if (!strcmp(name, #op)) {                                                                       \
    if (!edsp::args_ok(!strcmp(#op, "ge_scalarmult_base"), n, in, out)) return 1;                 \
    for (uint32_t i = 0; i < n; i++) edsp::l_##op(in + (uint64_t)i * NI, out + (uint64_t)i * NO, comb()); \
    return 0;                                                                                     \
  }
  EDSP_OPS(X)
#undef X
  return 2;
}

}  // extern "C"

#if defined(ED25519_SIGN_EMU_MAIN)
// records file: one record per line, "seedhex msghex pubhex sighex" with "-" for an empty field
static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return out;
}
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char sd[8192], m[8192], p[8192], s[8192];
  int n = 0, bad = 0;
  while (fscanf(f, "%8191s %8191s %8191s %8191s", sd, m, p, s) == 4) {
    const std::vector<uint8_t> seed = unhex(sd), msg = unhex(m), pub = unhex(p), sig = unhex(s);
    uint8_t got_pub[32], got_sig[64];
    const int st = emu_eds_signer(seed.data(), seed.size(), pub.size() == 32 ? pub.data() : nullptr, got_pub, nullptr);
    const int code = emu_eds_sign(seed.data(), seed.size(), msg.data(), msg.size(), got_sig);
    if (st != SIGNER_LOADED || code != (int)SIGN_OK || pub.size() != 32 || sig.size() != 64 ||
        memcmp(got_pub, pub.data(), 32) || memcmp(got_sig, sig.data(), 64)) {
      printf("record %d: status %d, code %d, or other bytes than expected\n", n, st, code);
      bad++;
    }
    n++;
  }
  fclose(f);
  printf("%d records, %d wrong\n", n, bad);
  return bad ? 1 : 0;
}
#endif
