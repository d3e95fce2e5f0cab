// k_rsa_digest512: SHA-384 or SHA-512 of n independent, variable-length,
// arbitrarily aligned messages -- the hashed RSA mode's front end for ring's
// RSA_PKCS1_2048_8192_SHA384 / _SHA512 and RSA_PKCS1_3072_8192_SHA384.  One
// kernel serves both digests: `digest` (wave-uniform) selects the initial
// values and how much of the state is output; the compression is shared.
// Record i gets T_i = DigestInfo prefix || H(msg_i) (67 or 83 bytes, at that
// stride) and t_offs[i] = stride i, which the unchanged raw RSA path
// (host_rsa.cpp rsa_run) takes as its (msgs, msg_offs); with prefix = 0 the
// 48- or 64-byte digests alone (cess_sha2_batch).
//
// Structure and contracts are k_rsa_digest's (read that file's header first):
// one wave per workgroup, one lane per message; per round the wave stages the
// next 256 bytes of each of its 64 messages into LDS, message m's 64 aligned
// dwords with one coalesced load whose parameters are scalars (v_readlane),
// kBatch messages' loads in flight at once; each lane then reads its own row,
// removes the misalignment with the byte funnel shift and adds the padding
// (rsa_digest512.hpp).  Loads stay inside the dwords that hold message bytes,
// idle lanes read the first dword of msg_offs, a record with unordered or
// out-of-range offsets hashes as empty.  What differs for the 64-bit hash:
//
// Round = 2 blocks.  The 256 staged bytes are two 128-byte blocks instead of
// four 64-byte ones; staging, the 65th ("carry") dword and the window
// arithmetic are unchanged, so a wave load still covers one message's 256
// contiguous bytes.
//
// LDS rows: stride 65 dwords, read with ds_read_b32.  What lies in LDS is the
// raw, misaligned byte stream as aligned dwords: a 64-bit message word starts
// at byte offset sh = 0..3 inside a dword and spans three of them, so LDS holds
// no aligned 64-bit quantity that a ds_read_b64 could deliver ready for use.
// The funnel shift works on neighbouring 32-bit dwords and yields the stream as
// 32-bit big-endian words; two of them are one message word (no further
// instruction: a register pair).  With 32-bit reads the bank rule is modulo 32
// over 32-lane halves: lane l reads dword 65 l + j, bank (l + j) mod 32, all
// different; the staging stores of a row are consecutive dwords.  An even
// stride (66, for 8-byte aligned ds_read_b64 at banks modulo 64: 2 l + 2 j,
// also conflict-free) would save half of the 64 LDS read instructions per
// round, against about 2 x 80 x 60 VALU instructions of compression, and cost
// 256 B of LDS; it was not worth a second layout.  64 x 65 x 4 = 16,640 B per
// workgroup: 9 workgroups per CU of 160 KiB, as k_rsa_digest.
//
// Compression in a 16-round loop body.  Fully unrolled, 80 rounds of
// two-instruction 64-bit operations are about 35 KB of code per call site,
// most of the 64 KB instruction cache that two CUs share; sha512_compress has
// rounds 0..15 straight and rounds 16..79 as four passes of one 16-round body
// instead (the kernel is 20 KB), with compile-time schedule indices (state
// 8 x u64 and schedule 16 x u64 stay in VGPRs) and the round constants fetched
// by scalar loads at a uniform address.  Rotations are two v_alignbit_b32 on
// the halves (named in rsa_digest512.hpp: from plain uint64_t shifts the
// compiler builds v_lshrrev_b64 / v_lshlrev_b64 / v_or triples); the 64-bit
// adds are plain C++, which the compiler turns into one v_lshl_add_u64 each.
// 138 VGPRs, no scratch: 3 waves per SIMD by registers, LDS (9 per CU) decides.
#include <hip/hip_runtime.h>

#include "rsa_digest512.hpp"

namespace {

constexpr int kRoundBlocks = 2;                  // 128-byte blocks per message and round
constexpr int kRoundWords = 32 * kRoundBlocks;   // = the wave's 64 lanes: one 32-bit stream word per lane
constexpr int kRowStride = kRoundWords + 1;      // dwords
constexpr int kBatch = 8;                        // messages whose loads are issued together
static_assert(kRoundWords == 64, "one stream word per lane");

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
}

}  // namespace

__global__ __launch_bounds__(64) void k_rsa_digest512(uint64_t n, const uint8_t* __restrict__ msgs,
                                                      const uint64_t* __restrict__ msg_offs,
                                                      uint8_t* __restrict__ out, uint32_t prefix,
                                                      uint64_t* __restrict__ t_offs, int digest) {
  using namespace rsa_digest;
  using namespace rsa_digest512;
  __shared__ uint32_t rows[64 * kRowStride];
  const uint32_t lane = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * 64 + lane;
  const uint32_t dlen = digest_len(digest), rec = (prefix ? kPrefixLen : 0) + dlen;
  uint64_t start = 0, len = 0;
  if (i < n) {
    const uint64_t total = msg_offs[n], b = msg_offs[i], e = msg_offs[i + 1];
    if (b <= e && e <= total) {
      start = b;
      len = e - b;
    }
  }
  if (t_offs && i <= n) t_offs[i] = (uint64_t)rec * i;
  const uint64_t nblk = i < n ? padded_len512(len) / 128 : 0;
  unsigned long long mx = nblk;
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const unsigned long long o = __shfl_xor(mx, off);
    mx = o > mx ? o : mx;
  }
  const uint32_t* safe = reinterpret_cast<const uint32_t*>(msg_offs);
  uint64_t st[8];
#pragma unroll
  for (int j = 0; j < 8; j++) st[j] = digest == kSha384 ? SHA384_IV[j] : SHA512_IV[j];

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
            blk[j] = stream_word512(r[j], r[j + 1], sh, avail, 128 * b + 4 * j, len, pos0);
        }
        sha512_compress(st, blk);
      }
    }
    __syncthreads();
  }

  // 64 records of rec bytes, assembled in LDS and written as consecutive dwords
  uint8_t* row = reinterpret_cast<uint8_t*>(rows) + rec * lane;
  if (prefix) {
#pragma unroll
    for (int j = 0; j < kPrefixLen; j++) row[j] = (uint8_t)prefix_byte(digest, j);
    row += kPrefixLen;
  }
#pragma unroll
  for (int j = 0; j < 64; j++)
    if ((uint32_t)j < dlen) row[j] = (uint8_t)(st[j >> 3] >> (56 - 8 * (j & 7)));
  __syncthreads();
  uint32_t* o32 = reinterpret_cast<uint32_t*>(out + (uint64_t)blockIdx.x * 64 * rec);
  for (uint32_t d = lane; d < 16 * rec; d += 64) o32[d] = rows[d];
}
