// prefix.h - the prefix filter (-p, ECL_PREFIX): "is this 160-bit value inside one of n ranges" in place of the bloom's "are these 20 bits set".
// (host and device: tests/test_prefix_host.py compiles these with g++ through csrc/tools/prefix_host.cpp)
//
// An address that starts with given characters is a hash160 inside one of a few inclusive ranges [lo, hi] (the host plans them:
// ecloop_amd/host/prefix_plan.h).  The table: n ranges of ten words, lo[5] then hi[5], most significant word first (h160_t's word order),
// sorted by lo and disjoint, 1 <= n <= 2^16.  The test has two stages, like the bloom's probe 0 and its rings:
//   stage 1 (every hash, in the hot loop): one plain load from a direct-mapped bitmap indexed by the leading PREFIX_BUCKET_BITS bits of
//     h[0]; a bucket's bit is set iff some range intersects the bucket.  2^24 buckets = 2 MiB: it stays in cache like a small filter.
//   exact stage (the ring's survivors, 64 at a time): a binary search for the last range with lo <= h, then h <= hi, all five words.
// A value is reported iff it lies inside a range: no false positives, and (the ranges are disjoint) no duplicates.
#pragma once
#include <stddef.h>
#include "fe256.h"

#define PREFIX_BUCKET_BITS 24u
#define PREFIX_MAX_RANGES (1u << 16)

// the 24 bytes of add_args' filter field in a prefix kernel (a union with bloom_t there: the kernarg layout of every kernel stays)
struct prefix_t {
  const u32* bitmap;  // 2^(32 - shift) bits
  const u32* table;   // n x 10 words
  u32 n;
  u32 shift;          // bucket of h = h[0] >> shift
};

FE_FN u32 prefix_bucket(const prefix_t& p, const u32 h[5]) { return h[0] >> p.shift; }
FE_FN bool prefix_stage1(const prefix_t& p, const u32 h[5]) {
  const u32 b = prefix_bucket(p, h);
  return (p.bitmap[b >> 5] >> (b & 31u)) & 1u;
}
// a <= b over five words, most significant first
FE_FN bool prefix_le(const u32* a, const u32* b) {
  bool le = true;  // (from the last word up: the most significant difference decides)
#pragma unroll
  for (int i = 4; i >= 0; --i) le = a[i] < b[i] || (a[i] == b[i] && le);
  return le;
}
// the exact test: the number of ranges with lo <= h by binary search (at most 17 steps), then h <= hi of the last of them
FE_FN bool prefix_exact(const prefix_t& p, const u32 h[5]) {
  u32 lo = 0, hi = p.n;  // ranges [0, lo) have lo <= h, ranges [hi, n) do not
  while (lo < hi) {
    const u32 mid = (lo + hi) >> 1;
    if (prefix_le(p.table + (size_t)mid * 10u, h)) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return false;
  return prefix_le(h, p.table + (size_t)(lo - 1) * 10u + 5u);
}
FE_FN bool prefix_has(const prefix_t& p, const u32 h[5]) { return prefix_stage1(p, h) && prefix_exact(p, h); }

// the bitmap of a table (host side of ecl_hip_set_bloom on a prefix context): bit b set iff a range intersects bucket b.
// bitmap: 2^(32 - shift) / 32 words, zeroed here.  The table must have passed prefix_table_ok.
inline void prefix_build_bitmap(u32* bitmap, const u32* table, u32 n, u32 shift) {
  const size_t words = ((size_t)1 << (32u - shift)) / 32u;
  for (size_t i = 0; i < words; ++i) bitmap[i] = 0;
  for (u32 r = 0; r < n; ++r) {
    const u32 b0 = table[(size_t)r * 10u] >> shift, b1 = table[(size_t)r * 10u + 5u] >> shift;
    u32 b = b0;
    // whole words in the middle of a long range, single bits at its ends
    while (b <= b1) {
      if ((b & 31u) == 0 && b1 - b >= 31u) {
        bitmap[b >> 5] = 0xFFFFFFFFu;
        if (b1 - b == 31u) break;
        b += 32u;
      } else {
        bitmap[b >> 5] |= 1u << (b & 31u);
        if (b == b1) break;
        ++b;
      }
    }
  }
}
// what ecl_hip_set_bloom accepts: 1 <= n <= 2^16, lo <= hi in every range, every lo above the hi before it
inline bool prefix_table_ok(const u32* table, unsigned long long n) {
  if (n == 0 || n > PREFIX_MAX_RANGES) return false;
  for (u32 r = 0; r < (u32)n; ++r) {
    const u32* e = table + (size_t)r * 10u;
    if (!prefix_le(e, e + 5)) return false;
    if (r && prefix_le(e, e - 5)) return false;  // unsorted or overlapping
  }
  return true;
}
