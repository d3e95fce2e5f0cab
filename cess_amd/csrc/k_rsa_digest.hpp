// The digest kernels: a SHA-2 hash of n independent, variable-length,
// arbitrarily aligned messages -- the hashed RSA mode's front end
// (RSASSA-PKCS1-v1_5, ring's RSA_PKCS1_2048_8192_SHA256 / _SHA384 / _SHA512 and
// RSA_PKCS1_3072_8192_SHA384) and Ed25519's hash.  k_rsa_digest.hip (SHA-256)
// and k_rsa_digest512.hip (SHA-384 and SHA-512: `digest`, wave-uniform, selects
// the initial values and how much of the state is output; the compression is
// shared) are one design over a hash description H (rsa_digest.hpp Sha256,
// rsa_digest512.hpp Sha512): this header holds that design's reasoning, its
// constants and readlane64, rsa_digest.hpp the message stream.
//
// Two bodies, kept alike by hand.  The body as one __device__ function
// template instantiated by both kernels computes the same and needs the same
// registers and LDS, but is no longer the parent's code: a function is
// optimised once on its own and again after inlining, which reorders the
// rounds' independent instructions, recomputes the last-block branch's
// position per word (SHA-256, +67 instructions) and splits the record's bytes
// less well (SHA-512, +27).  Both run once per message or wave, and on
// one-block messages the stage took 0.2-0.6 % longer, outside a run-to-run
// spread of 0.1-0.3 % (profiles/sha2_front_static.txt, sha2_front_ab.json).
// So each .hip file writes the body out with its block size; a change to one
// is made in the other.
//
// Output.  Record i gets T_i = DigestInfo prefix || H(msg_i) (19 + 32 / 48 / 64
// = 51 / 67 / 83 bytes, at that stride), which the unchanged raw RSA path
// (host_rsa.cpp rsa_run) then takes as its messages; with prefix = 0 the
// digests alone, at their own stride (cess_sha256_batch, cess_sha2_batch,
// Ed25519).  t_offs, where given, receives the n + 1 offsets stride i of those
// records.  The host passes t_offs only together with prefix (digest_run), so
// the stride it sees is T's.
//
// Layout: one wave per workgroup, one lane per message.  A lane walking its
// own message with byte loads would make every wave load touch 64 cache lines,
// so the wave stages cooperatively instead.  Per round it copies the next
// kRoundBlocks blocks (256 bytes: four 64-byte or two 128-byte ones) of each of
// its 64 messages into LDS: the 64 lanes fetch message m's 64 aligned dwords
// that cover those 256 bytes with one coalesced load and store them, as
// fetched, to row m (the message's start, length and shift are scalars of that
// iteration, v_readlane; kBatch messages' loads are in flight at once).  Each
// lane then reads its own row and turns the raw dwords into big-endian 32-bit
// stream words: a byte funnel shift over neighbouring dwords removes the
// misalignment (the 65th dword it needs at the end of a round, the "carry",
// comes from one per-lane load), and the blocks that hold the message's end get
// the SHA padding (rsa_digest.hpp).  It compresses kRoundBlocks blocks per
// round; state and schedule stay in VGPRs.
//
// Chunk size.  For SHA-256, state, schedule, a block's raw dwords and a batch
// of staged loads take about 115 VGPRs, so registers allow 4 waves per SIMD;
// LDS decides.  A row is 64 + 1 dwords: the odd stride puts the 32 lanes of a
// ds_read_b32 group on 32 different banks when they read word j of their rows
// (stride 65 = 1 mod 32), and the staging stores of one row are consecutive.
// 256 bytes per round make one wave load cover one message's 256 contiguous
// bytes (a full-width coalesced access, message parameters in SGPRs) at
// 64 x 65 x 4 = 16,640 B per wave: 9 waves per CU of 160 KiB, two per SIMD and
// one over, so a staging wave (latency-bound) has a compressing wave
// (VALU-bound) beside it.  Half of that would double the occupancy but halve
// the contiguous run and need per-lane message parameters; twice would leave
// one wave per SIMD.  The 64-bit hash keeps all of it: staging, the carry
// dword and the window arithmetic do not depend on the block size.
//
// LDS rows are read with ds_read_b32 for the 64-bit hash too.  What lies in
// LDS is the raw, misaligned byte stream as aligned dwords: a 64-bit message
// word starts at byte offset sh = 0..3 inside a dword and spans three of them,
// so LDS holds no aligned 64-bit quantity that a ds_read_b64 could deliver
// ready for use.  The funnel shift works on neighbouring 32-bit dwords and
// yields the stream as 32-bit big-endian words; two of them are one message
// word (no further instruction: a register pair).  With 32-bit reads the bank
// rule is modulo 32 over 32-lane halves: lane l reads dword 65 l + j, bank
// (l + j) mod 32, all different.  An even stride (66, for 8-byte aligned
// ds_read_b64 at banks modulo 64: 2 l + 2 j, also conflict-free) would save
// half of the 64 LDS read instructions per round, against about 2 x 80 x 60
// VALU instructions of compression, and cost 256 B of LDS; it was not worth a
// second layout.
//
// SHA-512's compression in a 16-round loop body.  Fully unrolled, 80 rounds of
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
//
// Lanes whose message has ended idle until the longest message of the wave is
// done: the wave's time is that of its longest message.  A batch with one very
// long record keeps that record's wave (and only it) busy for len / block
// compressions on a single lane; sorting or splitting such batches is the
// caller's business.
//
// Loads stay inside the dwords that hold message bytes (rsa_digest.hpp); lanes
// with nothing to fetch read the first dword of msg_offs instead, so the loads
// are unconditional and a batch of them is in flight at once.  A record whose
// offsets are not ordered or exceed msg_offs[n] is hashed as empty.
#pragma once
#include <hip/hip_runtime.h>

#include "rsa_digest.hpp"

namespace rsa_digest {

constexpr int kRoundWords = 64;               // stream words per message and round = the wave's lanes: one per lane
constexpr int kRowStride = kRoundWords + 1;   // dwords
constexpr int kBatch = 8;                     // messages whose loads are issued together

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
}

}  // namespace rsa_digest
