// The host layer's index arithmetic: no HIP and no context, so it also builds
// into a stand-alone CPU program (tests/hostemu/host_offsets_main.cpp, under
// the sanitizers).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "kernels.hpp"

namespace cess_host {

// bitmap words from codes (LSB first; bit i set iff record i verified)
inline void bitmap_from_codes(const uint8_t* codes, uint64_t n, uint64_t* words) {
  for (uint64_t w = 0; w < (n + 63) / 64; w++) words[w] = 0;
  for (uint64_t i = 0; i < n; i++)
    if (codes[i] == CODE_OK) words[i >> 6] |= 1ull << (i & 63);
}

// shard of a batch for rank r of R: whole bitmap words, equal word count per rank
inline void shard_of(uint64_t n, int nranks, int rank, uint64_t* begin, uint64_t* end, uint64_t* words_per_rank) {
  const uint64_t words = (n + 63) / 64;
  const uint64_t per = nranks > 0 ? (words + nranks - 1) / nranks : 0;
  const uint64_t b = std::min<uint64_t>(n, (uint64_t)rank * per * 64);
  const uint64_t e = std::min<uint64_t>(n, ((uint64_t)rank + 1) * per * 64);
  if (begin) *begin = b;
  if (end) *end = e;
  if (words_per_rank) *words_per_rank = per;
}

// Message offsets of records [off, off + m) of a batch (record i's bytes are
// [offs[i], offs[i + 1]) of the caller's buffer), rebased to the range's first
// byte: rebased[j] = offs[off + j] - offs[off], m + 1 entries; the range is
// bytes [*first, *first + *bytes).  False, with nothing to stage, if any pair
// of the range decreases (a record's length would wrap) or if the range is not
// empty and the caller has no byte buffer (have_bytes false).
inline bool rebase_offsets(const uint64_t* offs, uint64_t off, uint64_t m, bool have_bytes,
                           std::vector<uint64_t>& rebased, uint64_t* first, uint64_t* bytes) {
  const uint64_t* o = offs + off;
  rebased.resize(m + 1);
  for (uint64_t j = 0; j <= m; j++) {
    if (j && o[j] < o[j - 1]) return false;
    rebased[j] = o[j] - o[0];
  }
  *first = o[0];
  *bytes = rebased[m];
  return have_bytes || *bytes == 0;
}

}  // namespace cess_host
