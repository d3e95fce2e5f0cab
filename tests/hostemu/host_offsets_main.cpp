// Stand-alone CPU driver for the host layer's index arithmetic
// (cess_amd/csrc/host_pure.hpp): message-offset staging as the chunk loops of
// the host-buffer APIs drive it, the shard ranges and the bitmap words.
// Built with -fsanitize=address,undefined by tests/test_host_offsets.py; the
// offset arrays are heap vectors of exactly n + 1 entries, so a read past a
// chunk's range is reported.
#include <stdio.h>

#include "../../cess_amd/csrc/host_pure.hpp"

using namespace cess_host;

static int failures = 0;
#define CHECK(x)                                             \
  do {                                                       \
    if (!(x)) {                                              \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);    \
      failures++;                                            \
    }                                                        \
  } while (0)

// The host APIs' chunk loop over n records in chunks of cap: true if every
// chunk is accepted, and then every chunk's rebased offsets, first byte and
// byte count were checked against the definition.
static bool stage_all(const std::vector<uint64_t>& offs, uint64_t cap, bool have_bytes) {
  const uint64_t n = offs.size() - 1;
  std::vector<uint64_t> rebased;
  for (uint64_t off = 0; off < n; off += cap) {
    const uint64_t m = std::min(cap, n - off);
    uint64_t first = ~0ull, bytes = ~0ull;
    if (!rebase_offsets(offs.data(), off, m, have_bytes, rebased, &first, &bytes)) return false;
    CHECK(rebased.size() == m + 1);
    CHECK(first == offs[off]);
    CHECK(bytes == offs[off + m] - offs[off]);
    for (uint64_t j = 0; j <= m; j++) CHECK(rebased[j] == offs[off + j] - offs[off]);
    for (uint64_t j = 0; j < m; j++) CHECK(rebased[j + 1] - rebased[j] == offs[off + j + 1] - offs[off + j]);
  }
  return true;
}

// n records of lengths len(i), the first at byte `base`
template <class Len>
static std::vector<uint64_t> offsets(uint64_t n, uint64_t base, Len&& len) {
  std::vector<uint64_t> o(n + 1, base);
  for (uint64_t i = 0; i < n; i++) o[i + 1] = o[i] + len(i);
  return o;
}

static void test_offsets() {
  const uint64_t cap = 64;
  // m = 0: one entry, an empty range, accepted even without a byte buffer
  {
    std::vector<uint64_t> o = {7}, rebased;
    uint64_t first = 0, bytes = 1;
    CHECK(rebase_offsets(o.data(), 0, 0, false, rebased, &first, &bytes));
    CHECK(rebased.size() == 1 && rebased[0] == 0 && first == 7 && bytes == 0);
  }
  // one chunk; the first chunk ending exactly at cap and at cap + 1 records
  for (uint64_t n : {1ull, 5ull, 63ull, 64ull, 65ull, 129ull})
    CHECK(stage_all(offsets(n, 0, [](uint64_t i) { return 1 + i % 7; }), cap, true));
  // a non-zero offs[0]
  CHECK(stage_all(offsets(65, 1000, [](uint64_t i) { return 3 * (i % 5); }), cap, true));
  // runs of empty messages (a whole empty chunk among them)
  CHECK(stage_all(offsets(200, 5, [](uint64_t i) { return i >= 60 && i < 130 ? 0 : i % 3; }), cap, true));
  // a decreasing pair inside a chunk
  {
    std::vector<uint64_t> o = {0, 8, 4, 12};
    CHECK(!stage_all(o, cap, true));
    std::vector<uint64_t> p = offsets(130, 0, [](uint64_t) { return 4; });
    p[100] = p[99] - 1;   // second chunk
    CHECK(!stage_all(p, cap, true));
  }
  // a decreasing pair exactly across a chunk boundary: the last pair of the
  // first chunk, and the first pair of the second (the end points of both
  // chunks still increase)
  {
    std::vector<uint64_t> p = offsets(130, 0, [](uint64_t) { return 4; });
    p[64] = p[63] - 1;
    CHECK(!stage_all(p, cap, true));
    std::vector<uint64_t> q = offsets(130, 0, [](uint64_t) { return 4; });
    q[64] = q[65] + 1;   // offs[63] < offs[64] > offs[65]
    CHECK(q[0] < q[64] && q[64] < q[128]);
    CHECK(!stage_all(q, cap, true));
  }
  // offsets near 2^64 - 1
  {
    const uint64_t top = ~0ull;
    CHECK(stage_all({top - 10, top - 4, top - 4, top}, cap, true));
    CHECK(stage_all(offsets(65, top - 70, [](uint64_t) { return 1; }), cap, true));
    CHECK(!stage_all({top - 1, top, 0}, cap, true));   // the sum wrapped
    CHECK(!stage_all({top, 0}, cap, true));
  }
  // no byte buffer: accepted iff every chunk's range is empty
  CHECK(stage_all(offsets(130, 9, [](uint64_t) { return 0; }), cap, false));
  CHECK(!stage_all(offsets(130, 9, [](uint64_t i) { return i == 129 ? 1 : 0; }), cap, false));
  CHECK(!stage_all({0, 1}, cap, false));
}

static void test_shards() {
  for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 129ull, 4097ull})
    for (int nranks : {1, 2, 3, 8}) {
      uint64_t next = 0, wpr0 = 0;
      for (int r = 0; r < nranks; r++) {
        uint64_t b = ~0ull, e = ~0ull, wpr = ~0ull;
        shard_of(n, nranks, r, &b, &e, &wpr);
        if (r == 0) wpr0 = wpr;
        CHECK(wpr == wpr0);                 // one words_per_rank
        CHECK(b == next && b <= e);         // disjoint and in order, no gap
        CHECK(b % 64 == 0 || b == n);       // starts on a bitmap word (or is empty, at n)
        CHECK(e - b <= wpr * 64);
        CHECK(b == std::min<uint64_t>(n, (uint64_t)r * wpr * 64));
        next = e;
      }
      CHECK(next == n);                     // covers [0, n)
      CHECK((uint64_t)nranks * wpr0 * 64 >= n);
      // outputs are optional
      shard_of(n, nranks, 0, nullptr, nullptr, nullptr);
    }
}

static void test_bitmap() {
  const uint64_t n = 130;
  std::vector<uint8_t> codes(n);
  for (uint64_t i = 0; i < n; i++) codes[i] = i % 3 == 0 || i == 63 || i == 64 || i == 129 ? CODE_OK : 1 + i % 5;
  std::vector<uint64_t> words((n + 63) / 64, ~0ull);   // stale contents must be overwritten
  bitmap_from_codes(codes.data(), n, words.data());
  for (uint64_t i = 0; i < 64 * words.size(); i++)
    CHECK(((words[i / 64] >> (i % 64)) & 1) == (i < n && codes[i] == CODE_OK ? 1u : 0u));
  bitmap_from_codes(codes.data(), 0, nullptr);          // no record, no word
}

int main() {
  test_offsets();
  test_shards();
  test_bitmap();
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("OK: host offsets, shards, bitmap\n");
  return 0;
}
