// k_rsa_digest512: SHA-384 or SHA-512 (`digest`: CESS_RSA_DIGEST_SHA384 or
// _SHA512, wave-uniform) of n messages; T_i = DigestInfo prefix || H(msg_i)
// (67 or 83 bytes) or, with prefix = 0, the 48- or 64-byte digests alone
// (cess_sha2_batch, Ed25519).  Layout, contracts and reasoning:
// k_rsa_digest.hpp.  The body is k_rsa_digest.hip's for two 128-byte blocks
// per round.
#include "k_rsa_digest.hpp"
#include "rsa_digest512.hpp"

__global__ __launch_bounds__(64) void k_rsa_digest512(uint64_t n, const uint8_t* __restrict__ msgs,
                                                      const uint64_t* __restrict__ msg_offs,
                                                      uint8_t* __restrict__ out, uint32_t prefix,
                                                      uint64_t* __restrict__ t_offs, int digest) {
  using namespace rsa_digest;
  using H = rsa_digest512::Sha512;
  constexpr int kRoundBlocks = 2;
  __shared__ uint32_t rows[64 * kRowStride];
  const uint32_t lane = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * 64 + lane;
  const uint32_t dlen = H::digest_len(digest), rec = (prefix ? kPrefixLen : 0) + dlen;
  uint64_t start = 0, len = 0;
  if (i < n) {
    const uint64_t total = msg_offs[n], b = msg_offs[i], e = msg_offs[i + 1];
    if (b <= e && e <= total) {
      start = b;
      len = e - b;
    }
  }
  if (t_offs && i <= n) t_offs[i] = (uint64_t)rec * i;
  const uint64_t nblk = i < n ? padded_len<H>(len) / 128 : 0;
  unsigned long long mx = nblk;
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const unsigned long long o = __shfl_xor(mx, off);
    mx = o > mx ? o : mx;
  }
  const uint32_t* safe = reinterpret_cast<const uint32_t*>(msg_offs);
  uint64_t st[8];
#pragma unroll
  for (int j = 0; j < 8; j++) st[j] = H::iv(digest, j);

  const uint32_t sh = ((uint32_t)(uintptr_t)msgs + (uint32_t)start) & 3u;   // this lane's message
#pragma unroll 1
  for (uint64_t blk0 = 0; blk0 < mx; blk0 += kRoundBlocks) {
    const uint64_t pos0 = blk0 * 128;
    const uint32_t avail = window_avail(len, pos0);   // this lane's message
    // raw dword 64 of the lane's own window (the funnel shift of the round's
    // last word needs it): one per-lane load per round, in flight during staging
    const uint32_t carry =
        *(dword_needed(64, sh, avail) ? reinterpret_cast<const uint32_t*>(msgs + start + pos0 - sh) + 64 : safe);
#pragma unroll 1
    for (int m0 = 0; m0 < 64; m0 += kBatch) {
      uint32_t raw[kBatch];
      bool any = false;
#pragma unroll
      for (int u = 0; u < kBatch; u++) {   // message m0 + u: parameters in SGPRs, lane j fetches raw dword j
        const uint32_t m_avail = window_avail(readlane64(len, m0 + u), pos0);
        const uint8_t* a0 = msgs + readlane64(start, m0 + u) + pos0;
        const uint32_t m_sh = (uint32_t)(uintptr_t)a0 & 3u;
        any = any | (m_avail != 0);
        raw[u] = *(dword_needed(lane, m_sh, m_avail) ? reinterpret_cast<const uint32_t*>(a0 - m_sh) + lane : safe);
      }
      if (!any) continue;   // (wave-uniform) no message bytes of these messages in this round
#pragma unroll
      for (int u = 0; u < kBatch; u++) rows[(m0 + u) * kRowStride + lane] = raw[u];
    }
    __syncthreads();   // one wave: orders the staging stores before the row reads
#pragma unroll 1
    for (int b = 0; b < kRoundBlocks; b++) {
      if (blk0 + b < nblk) {
        const uint32_t* row = rows + lane * kRowStride + 32 * b;
        uint32_t r[33], blk[32];
#pragma unroll
        for (int j = 0; j < 32; j++) r[j] = row[j];
        r[32] = b == kRoundBlocks - 1 ? carry : row[32];
        if (128u * b + 128u <= avail) {   // the block lies inside the message: shift and swap only
#pragma unroll
          for (int j = 0; j < 32; j++)
            blk[j] = __builtin_bswap32((uint32_t)((((uint64_t)r[j + 1] << 32) | r[j]) >> (8 * sh)));
        } else {                          // the message's last bytes and the padding
#pragma unroll
          for (int j = 0; j < 32; j++)
            blk[j] = stream_word<H>(r[j], r[j + 1], sh, avail, 128 * b + 4 * j, len, pos0);
        }
        H::compress(st, blk);
      }
    }
    __syncthreads();
  }

  // 64 records of rec bytes, assembled in LDS and written as consecutive dwords
  uint8_t* row = reinterpret_cast<uint8_t*>(rows) + rec * lane;
  if (prefix) {
#pragma unroll
    for (int j = 0; j < kPrefixLen; j++) row[j] = (uint8_t)H::prefix_byte(digest, j);
    row += kPrefixLen;
  }
#pragma unroll
  for (int j = 0; j < 64; j++)
    if ((uint32_t)j < dlen) row[j] = (uint8_t)(st[j >> 3] >> (56 - 8 * (j & 7)));
  __syncthreads();
  uint32_t* o32 = reinterpret_cast<uint32_t*>(out + (uint64_t)blockIdx.x * 64 * rec);
  for (uint32_t d = lane; d < 16 * rec; d += 64) o32[d] = rows[d];
}
