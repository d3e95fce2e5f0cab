// RSASSA-PSS: the check after m = s^e mod n (ring's RSA_PSS_2048_8192_SHA256 /
// _SHA384 / _SHA512; rules and layout: rsa_pss.hpp).  One lane per record over
// a class list of k_rsa_classify / k_rsa_scatter, after the store-mode
// exponentiation kernel of that class (k_rsa_2048m.hip, k_rsa_2048um.hip,
// k_rsa_bigm.hip) has left m in `m` (word j of list entry t at m[j n_max + t])
// and RSA_MISMATCH, or its final RSA_SIG_RANGE, in codes.  Records that are in
// no list (KEY, SIG_LEN) and those with SIG_RANGE are not touched.
// One kernel per digest: SHA-256's needs far fewer registers than the 64-bit
// hashes', and a launch has one digest.
// mod_bits_rec, where given (cess_rsa_pss_em_batch: caller-supplied m, no key
// table), holds the modulus length of record r; else it is the key row's.
// digests: H(msg_r) as the digest kernels write it with prefix = 0.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "rsa_pss.hpp"

template <class P>
__device__ __forceinline__ void rsa_pss_lane(uint32_t n_max, const uint32_t* __restrict__ cnt,
                                             const uint32_t* __restrict__ rec, const uint32_t* __restrict__ key_idx,
                                             const RsaKeyDev* __restrict__ keys,
                                             const uint32_t* __restrict__ mod_bits_rec, const uint32_t* __restrict__ m,
                                             const uint32_t* __restrict__ digests, uint8_t* __restrict__ codes) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= *cnt || t >= n_max) return;
  const uint32_t r = rec[t];
  if (r == RSA_PAD) return;
  if (codes[r] == RSA_SIG_RANGE) return;
  uint32_t mod_bits, k;
  if (mod_bits_rec) {
    mod_bits = mod_bits_rec[r];
    k = (mod_bits + 7) / 8;
  } else {
    const RsaKeyDev& K = keys[key_idx[r]];
    mod_bits = K.mod_bits;
    k = K.k_bytes;
    if (k < 256) {   // ring's floor (2048 bits, the length rounded up to bytes): only another policy's table holds such a key
      codes[r] = RSA_KEY;
      return;
    }
  }
  const uint32_t nw = (k + 3) / 4;
  const uint32_t* mt = m + t;
  auto mw = [=](uint32_t j) { return j < nw ? mt[(uint64_t)j * n_max] : 0u; };
  uint32_t mh[P::kHW];
  const uint32_t* dg = digests + (uint64_t)r * P::kHW;
#pragma unroll
  for (int j = 0; j < P::kHW; j++) mh[j] = __builtin_bswap32(dg[j]);
  codes[r] = rsa_pss::check<P>(mw, mod_bits, k, mh);
}

#define CESS_RSA_PSS_KERNEL(NAME, P)                                                                                  \
  __global__ __launch_bounds__(256) void NAME(                                                                        \
      uint32_t n_max, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ rec,                             \
      const uint32_t* __restrict__ key_idx, const RsaKeyDev* __restrict__ keys,                                       \
      const uint32_t* __restrict__ mod_bits_rec, const uint32_t* __restrict__ m,                                      \
      const uint32_t* __restrict__ digests, uint8_t* __restrict__ codes) {                                            \
    rsa_pss_lane<P>(n_max, cnt, rec, key_idx, keys, mod_bits_rec, m, digests, codes);                                 \
  }
CESS_RSA_PSS_KERNEL(k_rsa_pss_sha256, rsa_pss::P256)
CESS_RSA_PSS_KERNEL(k_rsa_pss_sha384, rsa_pss::P384)
CESS_RSA_PSS_KERNEL(k_rsa_pss_sha512, rsa_pss::P512f)

// Keys of the 1024-bit size class have no store-mode kernel: ring's PSS
// algorithms reject every key below their floor of 2048 bits, so a table loaded
// under another policy gets RSA_KEY for such records: here for the 1024-bit
// class, in rsa_pss_lane for the shorter keys of the 2048-bit class.
__global__ __launch_bounds__(256) void k_rsa_pss_small(uint32_t n_max, const uint32_t* __restrict__ cnt,
                                                       const uint32_t* __restrict__ rec,
                                                       uint8_t* __restrict__ codes) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= *cnt || t >= n_max) return;
  const uint32_t r = rec[t];
  if (r != RSA_PAD) codes[r] = RSA_KEY;
}
