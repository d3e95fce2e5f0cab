// Host build of the RSASSA-PSS check (cess_amd/csrc/rsa_pss.hpp) and of the
// 2048-bit class's exponentiation in store mode (k_rsa.hpp STORE) for
// tests/test_rsa_pss.py: the EM check alone on caller-supplied m, and the one-
// record path -- exponentiation, m written out as words, EM check -- as
// k_rsa_verify_2048m followed by k_rsa_pss runs it.
// With -DRSA_PSS_EMU_MAIN the same entries run from a stand-alone program (for
// a build under the address and undefined-behaviour sanitizers): it reads the
// test's row file and writes one result word per row.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cess_amd/csrc/k_rsa.hpp"
#include "../../cess_amd/csrc/rsa_pss.hpp"

// m (em_len bytes, big-endian) as the kernels store it: little-endian words,
// word j at w[j * stride], exactly ceil(em_len / 4) of them
static std::vector<uint32_t> words_of(const uint8_t* em, uint32_t em_len, uint32_t stride) {
  const uint32_t nw = (em_len + 3) / 4;
  std::vector<uint32_t> w((size_t)nw * stride, 0);
  for (uint32_t i = 0; i < em_len; i++) w[(size_t)(i >> 2) * stride] |= (uint32_t)em[em_len - 1 - i] << (8 * (i & 3));
  return w;
}

// rules 4..8 on m = the em_len bytes at em (ring reads m to its end: a length
// other than k = ceil(mod_bits / 8) is a mismatch, decided by the host in
// cess_rsa_pss_em_batch as well); mhash: H(msg), digest_len(digest) bytes
extern "C" int emu_rsa_pss_em(int digest, uint32_t mod_bits, const uint8_t* em, uint32_t em_len,
                              const uint8_t* mhash) {
  const uint32_t h = rsa_pss::digest_len(digest);
  if (!h || mod_bits == 0 || mod_bits > 4112) return -1;   // (the largest key of the loop-form class)
  const uint32_t k = (mod_bits + 7) / 8;
  if (em_len != k) return RSA_MISMATCH;
  // exact-size copies, so that a read past either end is a sanitizer finding
  const std::vector<uint32_t> w = words_of(em, em_len, 3);
  std::vector<uint32_t> mh(h / 4);
  memcpy(mh.data(), mhash, h);
  return rsa_pss::check_stored(w.data(), 3, mod_bits, k, mh.data(), digest);
}

// one record of the 2048-bit class through rsa_verify_lane<RSA_L2048, false,
// true> (t = 0, cnt = 1) and the EM check on what it stored: the code
extern "C" int emu_rsa_pss_verify(int digest, uint32_t mod_bits, uint32_t k_bytes, uint64_t e, const uint32_t* n28,
                                  const uint32_t* r2_28, uint32_t ninv, const uint8_t* sig, const uint8_t* mhash) {
  const uint32_t h = rsa_pss::digest_len(digest);
  if (!h) return -1;
  constexpr int L = RSA_L2048, W = (28 * L + 31) / 32;
  std::vector<RsaKeyDev> keys(1);
  RsaKeyDev& K = keys[0];
  memset(&K, 0, sizeof(K));
  K.k_bytes = k_bytes, K.ninv = ninv, K.limbs = L, K.mod_bits = mod_bits, K.e = e;
  for (int i = 0; i < L; i++) K.n28[i] = n28[i], K.r2_28[i] = r2_28[i];
  const uint32_t rec[1] = {0}, key_idx[1] = {0};
  const uint64_t sig_offs[2] = {0, k_bytes};
  std::vector<uint8_t> s(sig, sig + k_bytes);
  std::vector<uint32_t> base(L), m(W, 0xa5a5a5a5u), mh(h / 4);
  memcpy(mh.data(), mhash, h);
  uint8_t codes[1] = {0xff};
  rsa_verify_lane<L, false, true>(0, 1, rec, key_idx, keys.data(), s.data(), sig_offs, nullptr, nullptr, base.data(),
                                  codes, m.data());
  if (codes[0] == RSA_SIG_RANGE) return RSA_SIG_RANGE;
  if (codes[0] != RSA_MISMATCH) return -2;   // the store mode's placeholder
  return rsa_pss::check_stored(m.data(), 1, mod_bits, k_bytes, mh.data(), digest);
}

#if defined(RSA_PSS_EMU_MAIN)
// rsa_pss_emu IN OUT.  IN is a sequence of rows of uint32 words:
//   kind 0: 0, digest, mod_bits, em_len, H(msg) (16 words, zero-padded), EM padded to whole words
//   kind 1: 1, digest, mod_bits, k_bytes, e low, e high, ninv, n (74), R^2 mod n (74), H(msg) (16 words),
//           the signature padded to whole words
// OUT takes one word per row.
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> in;
  uint32_t buf[4096];
  for (size_t got; (got = fread(buf, 4, 4096, f)) > 0;) in.insert(in.end(), buf, buf + got);
  fclose(f);
  std::vector<uint32_t> res;
  size_t p = 0;
  auto need = [&](size_t words) {
    if (p + words > in.size()) {
      fprintf(stderr, "truncated input\n");
      exit(2);
    }
  };
  while (p < in.size()) {
    need(4);
    const uint32_t kind = in[p], digest = in[p + 1], bits = in[p + 2], len = in[p + 3];
    p += 4;
    const uint32_t h = rsa_pss::digest_len((int)digest);
    if (!h || len > 1100) return 2;
    const size_t lw = (len + 3) / 4;
    if (kind == 0) {
      need(16 + lw);
      std::vector<uint8_t> mh(h), em(len);
      memcpy(mh.data(), &in[p], h);
      if (len) memcpy(em.data(), in.data() + p + 16, len);   // (an empty record: no bytes, and no pointer to copy to)
      p += 16 + lw;
      res.push_back((uint32_t)emu_rsa_pss_em((int)digest, bits, em.data(), len, mh.data()));
    } else if (kind == 1) {
      need(3 + 2 * RSA_L2048 + 16 + lw);
      const uint64_t e = (uint64_t)in[p] | (uint64_t)in[p + 1] << 32;
      const uint32_t ninv = in[p + 2];
      const std::vector<uint32_t> n(&in[p + 3], &in[p + 3] + RSA_L2048),
          r2(&in[p + 3 + RSA_L2048], &in[p + 3 + RSA_L2048] + RSA_L2048);
      p += 3 + 2 * RSA_L2048;
      std::vector<uint8_t> mh(h), sig(len);
      memcpy(mh.data(), &in[p], h);
      memcpy(sig.data(), in.data() + p + 16, len);
      p += 16 + lw;
      res.push_back((uint32_t)emu_rsa_pss_verify((int)digest, bits, len, e, n.data(), r2.data(), ninv, sig.data(),
                                                 mh.data()));
    } else {
      return 2;
    }
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(res.data(), 4, res.size(), f) != res.size() || fclose(f)) return 2;
  printf("%zu rows\n", res.size());
  return 0;
}
#endif
