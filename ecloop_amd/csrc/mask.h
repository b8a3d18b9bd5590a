// mask.h - the mask filter (-p 0xdead*beef, ECL_MASK): "do these bits of the 160-bit value have these values" in place of the prefix
// filter's "is the value inside a range".
// (host and device: tests/test_mask_host.py compiles these with g++ through csrc/tools/mask_host.cpp)
//
// An Ethereum address is plain hex without checksum characters, so a pattern with a suffix, both ends or holes is exactly a set of fixed
// bits (the host plans them: ecloop_amd/host/mask_plan.h).  The table: n entries of ten words, m[5] then v[5], most significant word first
// (h160_t's word order), v & ~m == 0 in every word, 1 <= n <= MASK_MAX_ENTRIES.  A value h is a member iff some entry has
// ((h[w] ^ v[w]) & m[w]) == 0 for all five words.  The test runs on every hash, in the hot loop, over all five words of every entry: it
// is exact - no false positive and no second stage - at one xor and one and-or per word and entry.  The entry index is wave-uniform:
// on the device the table is read through the constant address space (scalar loads, the entry's words are SGPR operands of the VALU).
#pragma once
#include <stddef.h>
#include "fe256.h"

#define MASK_MAX_ENTRIES 16u

// the 24 bytes of add_args' filter field in a mask kernel (a union with bloom_t and prefix_t there: the kernarg layout of every kernel stays)
struct mask_t {
  const u32* table;  // n x 10 words
  u32 n;
  u32 pad[3];
};

#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) u32* mask_ptr;
#define MASK_TABLE(t) ((mask_ptr)(uintptr_t)(t).table)
#else
typedef const u32* mask_ptr;
#define MASK_TABLE(t) ((t).table)
#endif

// one entry: the bits of h that differ from v under m, all five words folded into one
FE_FN u32 mask_entry_diff(mask_ptr e, const u32 h[5]) {
  u32 d = 0;
#pragma unroll
  for (int w = 0; w < 5; ++w) {
    // one SGPR operand per instruction (v_xor, then v_and_or on the running d): fused into a three-operand bit operation the compiler
    // reads two, which the VALU cannot, and spends a move and a register per word on it
    u32 x = h[w] ^ e[5 + w];
    FE_HIDE24(x);
    d |= x & e[w];
    FE_HIDE24(d);
  }
  return d;
}
FE_FN bool mask_has(const mask_t& t, const u32 h[5]) {
  const mask_ptr tab = MASK_TABLE(t);
  // (the least difference over the entries, compared once: a flag per entry would be a compare and three mask operations on the scalar
  // unit per entry, and two more SGPR pairs live across the loop)
  // One entry per iteration, from the last one down by its word offset: the loop then holds one entry's ten words, the offset and the
  // address in SGPRs.  Two entries per iteration (the compiler's choice when left alone) and a pointer walked beside a counter each cost
  // the -endo kernel SGPR spills, and with them a VGPR to keep them in.
  u32 least = ~0u;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (u32 at = t.n * 10u; at != 0;) {
    at -= 10u;
    const u32 d = mask_entry_diff(tab + at, h);
    least = d < least ? d : least;
  }
  return least == 0;
}

// what ecl_hip_set_bloom accepts on a mask context: 1 <= n <= 16, no value bit outside its mask, no two identical entries.  An all-zero
// mask is legal here (it matches every value: the self-test uses it); how much of the space a table may cover is the planner's business
inline bool mask_table_ok(const u32* table, unsigned long long n) {
  if (n == 0 || n > MASK_MAX_ENTRIES) return false;
  for (u32 r = 0; r < (u32)n; ++r) {
    const u32* e = table + (size_t)r * 10u;
    for (int w = 0; w < 5; ++w)
      if (e[5 + w] & ~e[w]) return false;
    for (u32 q = 0; q < r; ++q) {
      const u32* f = table + (size_t)q * 10u;
      bool same = true;
      for (int w = 0; w < 10; ++w) same = same && e[w] == f[w];
      if (same) return false;
    }
  }
  return true;
}
