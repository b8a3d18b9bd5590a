/* kangaroo_plan.h - the arithmetic of the `kangaroo` command: Pollard's lambda (kangaroo) search for the private key of a KNOWN public key
   Q = key G with a <= key <= b.  Plain C, no GPU: the library (csrc/abi_herd.h), the CLI (cli_kangaroo.h) and the host test program
   (csrc/tools/kangaroo_host.cpp) all include this file, so the code that is tested is the code that runs.  THIS FILE IS THE DEFINITION of
   the method: the library, engine.py and tests/kangaroo_ref.py agree with it bit for bit.

   The method.  A herd of H = 2^herd_log2 kangaroos; kangaroo i is tame if i is even and wild if i is odd.
     Stream: SplitMix64 of `seed` (kg_next).  A 128-bit draw takes two outputs, the first the low half (kg_draw).
     Jump distances: s_j, j < 32, drawn first: s_j = 1 + (v mod 2^(jb + 1)); a draw that equals an earlier s is drawn again, so all 32
       differ (they are below n / 2, so the 32 table points T_j = s_j G have 32 different x).  jb = 4 ... 120: below 4 there are fewer than 32 values.
     Start offsets: r_i, i < H, drawn after the table: r_i = v mod 2^sb.
     Starts: tame i at (B + r_i) G, wild i at Q + r_i G (the complete addition), both with distance r_i.  A start that is the point at
       infinity fails the call (ECL_E_RANGE).
     A jump: with x canonical, j = bits 32..36 of x; P <- P + T_j, d <- d + s_j.  If x(P) = x(T_j) the sum would be a doubling or the point
       at infinity: the kangaroo takes j + 1 mod 32 for this jump instead (x(T_j) != x(T_j+1), so that one is an ordinary addition).
     Distinguished point: after a jump, the low dp bits of x are zero.  Its record carries the herd (tame / wild), the 128-bit distance and
       the identity, the leading 96 bits of x.  A distance that would pass 2^128 fails the call.
     Collision: a tame point (B + d_t) G and a wild point Q + d_w G with the same x mean key = B + d_t - d_w or key = -(B + d_t) - d_w
       (mod n) - kg_candidates; the driver re-derives both and accepts only the one whose point is Q.
   The driver (the CLI's, engine.kangaroo_search's and the yardstick's are the same): rounds of round_steps jumps per kangaroo, one device
   call each; the round's records sorted by (identity, distance, herd) and put one by one into a table keyed on the identity: a new
   identity is stored (dps), a stored one of the same herd is counted (same_herd) and the stored record kept, one of the other herd gives
   the two candidates, checked in the order of kg_candidates (candidates_checked counts every check) - the first that is Q's ends the
   search.  After a round that found nothing, the search gives up once the jumps made reach kg_give_up. */
#ifndef KANGAROO_PLAN_H
#define KANGAROO_PLAN_H
#include "bsgs_plan.h" /* bsgs_int and its arithmetic, n, the lift of a compressed key, the curve check */

#define KG_OK 0
#define KG_E_ORDER 1 /* a = 0, a > b or b >= n */
#define KG_E_WIDTH 2 /* b - a + 1 above 2^124 */
#define KG_E_OPT 3   /* herd_log2 outside 1 ... 24 or dp above 32 */
#define KG_TABLE 32u
#define KG_HERD_LOG2_MAX 24u
#define KG_DP_MAX 32u
#define KG_JB_MIN 4u /* 2^(jb + 1) values hold 32 different distances only from jb = 4 on */
#define KG_JB_MAX 120u
#define KG_SB_MAX 124u
#define KG_STORE_LOG2 26u /* dp's default keeps the expected number of stored points below about 2^26 */

typedef struct { uint64_t s; } kg_stream;
typedef struct { uint64_t lo, hi; } kg_u128;

static inline uint64_t kg_next(kg_stream *st) {
  uint64_t z = (st->s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
/* v mod 2^bits, bits = 1 ... 128: two outputs, the first is the low half */
static inline kg_u128 kg_draw(kg_stream *st, unsigned bits) {
  kg_u128 v;
  v.lo = kg_next(st), v.hi = kg_next(st);
  if (bits < 64) v.lo &= (1ull << bits) - 1, v.hi = 0;
  else if (bits < 128) v.hi &= bits == 64 ? 0 : (1ull << (bits - 64)) - 1;
  return v;
}
/* the 32 jump distances, all different, each 1 ... 2^(jb + 1); jb >= KG_JB_MIN (the caller checks: with fewer values this would not end) */
static inline void kg_table(kg_stream *st, unsigned jb, kg_u128 s[KG_TABLE]) {
  for (unsigned j = 0; j < KG_TABLE;) {
    kg_u128 v = kg_draw(st, jb + 1);
    if (++v.lo == 0) ++v.hi; /* jb + 1 <= 121: no carry out of the high half */
    unsigned k = 0;
    while (k < j && (s[k].lo != v.lo || s[k].hi != v.hi)) ++k;
    if (k == j) s[j++] = v;
  }
}
static inline kg_u128 kg_offset(kg_stream *st, unsigned sb) { return kg_draw(st, sb); }

typedef struct {
  bsgs_int a, b, base;   /* the range; B, the base scalar of the tame herd (= a: the tame starts lie over [a, a + 2^sb)) */
  unsigned wbits;        /* bits of W = b - a + 1: the bit length of W - 1 (0 for W = 1, k for W = 2^k) */
  unsigned herd_log2, dp, jb, sb;
  uint64_t round_steps;  /* jumps per kangaroo and round (device call) of the driver's default */
} kg_plan;

static inline unsigned kg_clamp(int v, unsigned lo, unsigned hi) { return v < (int)lo ? lo : v > (int)hi ? hi : (unsigned)v; }
/* everything from (a, b); herd_log2 / dp < 0: the defaults.
     herd_log2 = wbits / 2 - 4 in 1 ... 22: a kangaroo then makes about 32 jumps before the herds are expected to meet;
     jb = wbits / 2 + herd_log2 - 2 in 4 ... 120: the mean jump is about sqrt(W) H / 4, the usual choice for H walkers;
     sb = wbits in 1 ... 124;
     dp = wbits / 2 - herd_log2 - 1 (the H 2^dp jumps a herd needs to reach its distinguished points stay a fraction of the 2 sqrt(W) expected),
       raised to wbits / 2 + 2 - 26 where 4 sqrt(W) / 2^dp stored points would pass 2^26; 0 ... 32;
     round_steps = 2^(wbits / 2 - 1 - herd_log2): a round is about sqrt(W) / 2 jumps, at least one step and at most 2^34 jumps. */
static inline int kg_plan_make(kg_plan *p, const bsgs_int *a, const bsgs_int *b, int herd_log2, int dp) {
  const bsgs_int zero = {{0, 0, 0, 0}};
  if (bsgs_cmp(a, &zero) == 0 || bsgs_cmp(a, b) > 0 || bsgs_cmp(b, &BSGS_N) >= 0) return KG_E_ORDER;
  memset(p, 0, sizeof *p);
  bsgs_int w1;
  bsgs_sub(&w1, b, a); /* W - 1 */
  p->a = *a, p->b = *b, p->base = *a, p->wbits = bsgs_bits(&w1);
  if (p->wbits > 124) return KG_E_WIDTH;
  if (herd_log2 >= 0 && (herd_log2 < 1 || herd_log2 > (int)KG_HERD_LOG2_MAX)) return KG_E_OPT;
  if (dp > (int)KG_DP_MAX) return KG_E_OPT;
  const int half = (int)(p->wbits / 2);
  p->herd_log2 = herd_log2 >= 0 ? (unsigned)herd_log2 : kg_clamp(half - 4, 1, 22);
  p->jb = kg_clamp(half + (int)p->herd_log2 - 2, KG_JB_MIN, KG_JB_MAX);
  p->sb = kg_clamp((int)p->wbits, 1, KG_SB_MAX);
  if (dp >= 0) p->dp = (unsigned)dp;
  else {
    int d = half - (int)p->herd_log2 - 1, floor_ = half + 2 - (int)KG_STORE_LOG2;
    p->dp = kg_clamp(d > floor_ ? d : floor_, 0, KG_DP_MAX);
  }
  const int rs = half - 1 - (int)p->herd_log2, rmax = 34 - (int)p->herd_log2;
  p->round_steps = 1ull << kg_clamp(rs < rmax ? rs : rmax, 0, 33);
  return KG_OK;
}
/* the give-up limit in jumps: max_factor * 2 sqrt(W) + H 2^dp with sqrt(W) taken as 2^ceil(wbits / 2); 128 bits (max_factor < 2^32) */
static inline kg_u128 kg_give_up(const kg_plan *p, uint32_t max_factor) {
  const unsigned __int128 v = ((unsigned __int128)max_factor << (1 + (p->wbits + 1) / 2)) + ((unsigned __int128)1 << (p->herd_log2 + p->dp));
  kg_u128 r = {(uint64_t)v, (uint64_t)(v >> 64)};
  return r;
}
/* the two keys a tame / wild pair with equal identity stands for: k1 = B + d_t - d_w, k2 = -(B + d_t) - d_w  (mod n); B < n, d < 2^128 */
static inline void kg_candidates(bsgs_int *k1, bsgs_int *k2, const bsgs_int *base, kg_u128 dt, kg_u128 dw) {
  const bsgs_int zero = {{0, 0, 0, 0}}, t = {{dt.lo, dt.hi, 0, 0}}, w = {{dw.lo, dw.hi, 0, 0}};
  bsgs_int e, m;
  if (bsgs_add(&e, base, &t) || bsgs_cmp(&e, &BSGS_N) >= 0) bsgs_sub(&e, &e, &BSGS_N); /* B + d_t mod n (n > 2^255: once is enough) */
  if (bsgs_sub(k1, &e, &w)) bsgs_add(k1, k1, &BSGS_N);
  if (bsgs_cmp(&e, &zero) == 0) m = zero;
  else bsgs_sub(&m, &BSGS_N, &e);
  if (bsgs_sub(k2, &m, &w)) bsgs_add(k2, k2, &BSGS_N);
}
/* the sixteen limbs an ECL_PUB | ECL_HERD context takes as `start` (include/ecloop_hip.h) */
static inline void kg_block(uint64_t blk[16], const kg_plan *p, const uint64_t qx[4], const uint64_t qy[4], uint64_t seed) {
  memcpy(blk, p->base.w, 32), memcpy(blk + 4, qx, 32), memcpy(blk + 8, qy, 32);
  blk[12] = seed, blk[13] = p->herd_log2, blk[14] = p->jb, blk[15] = p->sb;
}
#endif
