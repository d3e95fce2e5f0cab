// Host build of k_rsa_verify_big (cess_amd/csrc/k_rsa_big.hip), the kernel
// source itself with the launch keywords defined away and thread 0 of block 0
// as the only thread, for tests/hostemu/rsa_emu.cpp (emu_rsa_verify at
// L > 74).  A translation unit of its own: k_rsa_big.hip and k_rsa.hpp each
// bring their namespace's M28 into the global scope.
#include <stdint.h>
#include <string.h>

#include <vector>

namespace {
struct EmuDim {
  uint32_t x, y, z;
};
const EmuDim blockIdx{0, 0, 0}, blockDim{256, 1, 1}, threadIdx{0, 0, 0};
}  // namespace
#define __global__ static
#define __launch_bounds__(...)
#include "../../cess_amd/csrc/k_rsa_big.hip"

// one record through the kernel (*cnt = 1, n_max = 1): the code, 0xff if none
// was written
extern "C" int emu_rsa_verify_big(int L, uint32_t k_bytes, uint64_t e, const uint32_t* n28, const uint32_t* r2_28,
                                  uint32_t ninv, const uint8_t* sig, const uint8_t* msg, uint32_t msg_len) {
  if (L <= 0 || L > RSA_LMAX) return -1;
  std::vector<RsaKeyDev> keys(1);
  RsaKeyDev& K = keys[0];
  memset(&K, 0, sizeof(K));
  K.k_bytes = k_bytes, K.ninv = ninv, K.limbs = (uint32_t)L, K.e = e;
  for (int i = 0; i < L; i++) K.n28[i] = n28[i], K.r2_28[i] = r2_28[i];
  const uint32_t cnt = 1, rec[1] = {0}, key_idx[1] = {0};
  const uint64_t sig_offs[2] = {0, k_bytes}, msg_offs[2] = {0, msg_len};
  // exact-size copies, so that a read past either end is a sanitizer finding
  std::vector<uint8_t> s(sig, sig + k_bytes), m(msg, msg + msg_len);
  uint8_t codes[1] = {0xff};
  k_rsa_verify_big(1, &cnt, rec, key_idx, keys.data(), s.data(), sig_offs, m.data(), msg_offs, codes);
  return codes[0];
}
