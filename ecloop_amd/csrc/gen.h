// gen.h — the candidates of an ECL_GEN context (`brain`): the template's expansion on the device.  The template and the order of its
// candidates are defined in host/gen_plan.h; no reference counterpart.
//
// k_gen_lines writes the m candidates first ... first + m - 1 of a piece as text and line table, where k_raw_scalars* then reads them as
// it reads the lines of `mul -raw`: candidate j at byte text_at + j * stride of the device text (stride = L rounded up to whole words,
// a slot per candidate whatever its length), its table entry start | length << 32.  Each thread takes GEN_R consecutive candidates: it
// takes the digits of its first index by division (64 bits while the quotient needs them) and then steps them like an odometer, the last
// position fastest.  A candidate is assembled in a 64-bit funnel - the alternative's bytes are gathered four at a time from the pool,
// any alignment, as the hashing kernels gather a line - and leaves as whole words: a slot is written by one thread only, so there are
// no byte stores and no atomics; the bytes of a slot behind the candidate's last word keep what they held (the hash reads a line by its
// length).  No barrier, no LDS; the loop bounds are the position count (a kernel argument) and the alternatives' lengths.
//
// The table on the device is the blob as the host holds it, behind it two spare words (the gather reads one word past the last byte):
// pos[] and alt[] are word-aligned there, counts and first alternatives also travel as kernel arguments (scalar registers).
#pragma once
#include "fe256.h"
#include <stddef.h>

#define GEN_R 4u          /* candidates per thread */
#define GEN_POSITIONS 16  /* host/gen_plan.h: GEN_POS_MAX */

struct gen_args {
  u32 npos;
  u32 alt_word;   // word offset of alt[] in the table
  u32 pool_byte;  // byte offset of the pool in the table
  u32 count[GEN_POSITIONS], first[GEN_POSITIONS];
};

// What the host side derives from an accepted template (host/gen_plan.h's gen_info), in one place for the library (abi_gen.h) and the host
// harness (tools/gen_host.cpp): the kernel's arguments, the bytes of a candidate's slot in the device text - the longest candidate in
// whole words, at least one - and the words of the table as the device holds it: the blob, then two spare words (gen_gather reads one
// word past the byte it is asked for).
static inline gen_args gen_args_make(u32 npos, u32 alt_at, u32 pool_at, const u32* count, const u32* first) {
  gen_args g = {};
  g.npos = npos, g.alt_word = alt_at / 4u, g.pool_byte = pool_at;
  for (u32 p = 0; p < npos && p < GEN_POSITIONS; ++p) g.count[p] = count[p], g.first[p] = first[p];
  return g;
}
static inline u32 gen_stride_bytes(u32 L) { return L ? (L + 3u) & ~3u : 4u; }
static inline size_t gen_table_words(size_t blob_bytes) { return (blob_bytes + 3) / 4 + 2; }

// the digits of index i: i = sum d[p] * prod_{q > p} count[q]
FE_FN void gen_digits(const gen_args& g, u64 i, u32 d[GEN_POSITIONS]) {
#pragma unroll
  for (int p = GEN_POSITIONS - 1; p >= 0; --p) {
    d[p] = 0;
    if ((u32)p < g.npos) {
      const u32 c = g.count[p];
      if (i >> 32) {
        const u64 q = i / c;
        d[p] = (u32)(i - q * c), i = q;
      } else {
        const u32 lo = (u32)i, q = lo / c;
        d[p] = lo - q * c, i = q;
      }
    }
  }
}
// the digits of the next index (the last candidate of all wraps to the first: its caller never reads past T)
FE_FN void gen_step(const gen_args& g, u32 d[GEN_POSITIONS]) {
  bool carry = true;
#pragma unroll
  for (int p = GEN_POSITIONS - 1; p >= 0; --p)
    if ((u32)p < g.npos && carry) {
      const u32 v = d[p] + 1u;
      carry = v == g.count[p];
      d[p] = carry ? 0u : v;
    }
}
// the four bytes of the table at byte offset `at`, first byte lowest
FE_FN u32 gen_gather(const u32* __restrict__ tab, u32 at) {
  const u32 sh = (at & 3u) * 8u;
  const u32 lo = tab[at >> 2], hi = tab[(at >> 2) + 1];
  return (u32)((((u64)hi << 32) | lo) >> sh);
}
// the candidate of the digits d into the words at `out` (room for out_words of them: nothing is written behind): -> its length in bytes
FE_FN u32 gen_expand(const u32* __restrict__ tab, const gen_args& g, const u32 d[GEN_POSITIONS], u32* __restrict__ out, u32 out_words) {
  u64 acc = 0;        // bytes that have not left yet, first byte lowest
  u32 pending = 0;    // how many: below 4 between two alternatives' words
  u32 words = 0, len = 0;
#pragma unroll
  for (int p = 0; p < GEN_POSITIONS; ++p)
    if ((u32)p < g.npos) {
      const u32* e = tab + g.alt_word + 2u * (g.first[p] + d[p]);
      const u32 off = g.pool_byte + e[0], l = e[1];
#pragma unroll 1
      for (u32 k = 0; k < l; k += 4u) {
        u32 v = gen_gather(tab, off + k);
        const u32 take = l - k < 4u ? l - k : 4u;
        if (take < 4u) v &= 0xFFFFFFFFu >> (32u - 8u * take);
        acc |= (u64)v << (8u * pending);
        pending += take;
        if (pending >= 4u) {
          if (words < out_words) out[words] = (u32)acc;
          ++words, acc >>= 32, pending -= 4u;
        }
      }
      len += l;
    }
  if (pending && words < out_words) out[words] = (u32)acc;
  return len;
}
// what thread t of a launch over m candidates does (the kernel's body; csrc/tools/gen_host.cpp runs it on the host)
FE_FN void gen_thread(const u32* __restrict__ tab, const gen_args& g, u64 first, u32 m, u32 t, u32 stride, u32 text_at, u32* __restrict__ text,
                      u64* __restrict__ lines) {
  const u64 j0 = (u64)t * GEN_R;
  if (j0 >= m) return;
  u32 d[GEN_POSITIONS];
  gen_digits(g, first + j0, d);
#pragma unroll 1
  for (u32 r = 0; r < GEN_R; ++r) {
    const u32 j = (u32)j0 + r;
    if (j >= m) break;
    const u32 at = text_at + j * stride;  // (below 2^32: the host sizes the regions)
    const u32 len = gen_expand(tab, g, d, text + (at >> 2), stride >> 2);
    lines[j] = (u64)at | (u64)len << 32;
    gen_step(g, d);
  }
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(256) k_gen_lines(const u32* __restrict__ tab, gen_args g, u64 first, u32 m, u32 stride, u32 text_at, u32* __restrict__ text,
                                                    u64* __restrict__ lines) {
  gen_thread(tab, g, first, m, blockIdx.x * 256u + threadIdx.x, stride, text_at, text, lines);
}
#endif
