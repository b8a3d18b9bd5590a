// add_kernel.h — the `add` hot loop on gfx950: batch affine point addition + hash160 + bloom probe, fused.
//
// Replaces batch_add + check_found_add of the reference (main.c:287-403) together with everything they call
// (fe_modp_grpinv lib/ecc.c:522-540, addr33/65_batch lib/addr.c:99-131, blf_has lib/utils.c:308-326).
//
// Same mathematics as the reference: a group of 2B consecutive keys around a centre point C is produced as
// C, C + G_i (i < B-1) and C - G_i (i < B) with G_i = (i+1)*stride*G taken from a precomputed table, using ONE
// field inversion for all B differences (Montgomery's trick); the next centre comes from one more addition.
// Re-designed for the GPU:
//   * one lane = one walk (its own centre), all lanes of the grid add the SAME table point in the same
//     iteration, so the table operand is wave-uniform (scalar loads / SGPR operands);
//   * the lane's chain of prefix products lives in HBM in a lane-interleaved layout (16 B per lane per
//     access -> 1 KiB coalesced per wave instruction), B x 32 B per lane: 288 GB of HBM makes a deep chain
//     cheap, so the inversion cost per key (270 mults / 2B keys) is small without any cross-lane exchange;
//   * the step to the next centre is folded into the same batched inversion as chain element 0, so there is
//     no separate full inversion per group (the reference pays one, main.c:400);
//   * walks are interleaved: lane g of T handles groups g, g+T, g+2T, ... so a contiguous follow-up call
//     continues from the centres left in HBM without any new scalar multiplication;
//   * hashing and the bloom probe run in the same kernel on the just-computed (x, y): points never go to HBM.
// Key order inside a group follows the reference (main.c:388-391): offset 0..B-1 = C - G_{B-1-j},
// offset B = C, offset B+1+i = C + G_i.
#pragma once
#include "bloom.h"
#include "emit33.h"
#include "hash160.h"
#include "keccak.h"
#include "pub_emit.h"
#include "prefix.h"
#include "mask.h"

struct ecl_found_dev {
  u64 key_offset;
  u32 h160[5];
  u32 tag;  // byte 0 = endo, byte 1 = address type (ecl_found.compressed: 1 addr33, 0 addr65, 2 p2sh, 3 eth, 4 p2tr, 5 pub)
};

struct add_args {
  const u32* __restrict__ tab;  // [B][ECL_TAB_STRIDE]: limbs x[9], y[9] of (i+1)*stride*G (normalised 9x29), 2 words pad
  u32 jump[16];                 // x[8], y[8] of (T*2B*stride)*G
  uint4* __restrict__ cxy;      // lane centres as canonical words, planes {x.lo, x.hi, y.lo, y.hi} x T
  uint4* __restrict__ scratch;  // prefix products (9x29 limbs 0..7), [(k*2 + half) * T + lane]
  u32* __restrict__ scratch2;   // prefix products (limb 8), [k * T + lane]
  union {
    bloom_t bloom;
    prefix_t prefix;  // the prefix kernels (k_add_pfx, k_add_pfx_eth): bitmap, range table, n, bucket shift in the same 24 bytes
    mask_t mask;      // the mask kernels (k_add_msk_eth): table, n, padding in the same 24 bytes
  };
  union {
    ecl_found_dev* found;
    u32* slab;  // the Taproot emit kernels (no filter, no records): where the points and tweaks go, TR_SLAB_WORDS words per key (tr_emit)
  };
  u32* counter;
  union {
    u32 cap;
    u32 epoch;  // the Taproot emit kernels: 0 / 1, the mark of this launch's slab entries
  };
  u32 B;      // table points per group (group = 2B keys)
  u32 T;      // lanes
  u32 nb;     // groups per lane in this launch
  u64 nkeys;  // keys with offset >= nkeys are not tested
  unsigned long long* keys;  // the call's key count (cand_queues::keys): each wave adds what reached check_point, once, at its end
};

// canonical words in two uint4 planes <-> fe
FE_FN fe fe_ld_words2(const uint4* p, size_t stride) {
  uint4 lo = p[0], hi = p[stride];
  const u32 w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return fe_from_words(w);
}
FE_FN void fe_st_words2(uint4* p, size_t stride, fe a) {  // normalises
  fe_normalize(a);
  u32 w[8];
  fe_to_words(w, a);
  p[0] = make_uint4(w[0], w[1], w[2], w[3]);
  p[stride] = make_uint4(w[4], w[5], w[6], w[7]);
}
// raw limbs (any magnitude) in planes uint4, uint4, u32.  These are the prefix-product chain's accesses: every element is
// written once and read once, a whole group later - a stream with no reuse in any cache.  It does not hurt the filter's
// cache residency either: non-temporal loads / stores measured 0.2 % / 1.8 % slower (profiles/r03_nt_ab.txt), so they stay plain.
FE_FN fe fe_ld_limbs(const uint4* p4, size_t stride4, const u32* p1) {
  fe r;
  const uint4 a = p4[0], b = p4[stride4];
  r.n[8] = p1[0];
  r.n[0] = a.x, r.n[1] = a.y, r.n[2] = a.z, r.n[3] = a.w;
  r.n[4] = b.x, r.n[5] = b.y, r.n[6] = b.z, r.n[7] = b.w;
  return r;
}
FE_FN void fe_st_limbs(uint4* p4, size_t stride4, u32* p1, const fe& a) {
  p4[0] = make_uint4(a.n[0], a.n[1], a.n[2], a.n[3]);
  p4[stride4] = make_uint4(a.n[4], a.n[5], a.n[6], a.n[7]);
  p1[0] = a.n[8];
}
// Table entries are read through the constant address space: the address is wave-uniform (kernel argument + loop
// counter), so these become scalar loads (s_load_dwordx*) into SGPRs and everything computed from them alone
// (negation, X-independent sums) runs on the scalar unit; the limbs are stored ready-made so there is nothing to
// convert.  The table is written by an earlier kernel and never by this one.
#define ECL_TAB_STRIDE 20u
typedef const __attribute__((address_space(4))) u32* ctab_ptr;
__device__ __forceinline__ fe fe_ld_tab(ctab_ptr p) {
  fe r;
#pragma unroll
  for (int i = 0; i < FE_LIMBS; ++i) r.n[i] = p[i];
  return r;
}
// 8 canonical words at p (argument data) -> fe
FE_FN fe fe_ldw(const u32* p) {
  u32 w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = p[i];
  return fe_from_words(w);
}

__device__ __forceinline__ void found_push(const add_args& a, u64 off, const u32 h[5], u32 endo, u32 compressed) {
  u32 idx = atomicAdd(a.counter, 1u);
  if (idx < a.cap) {
    ecl_found_dev r;
    r.key_offset = off;
#pragma unroll
    for (int i = 0; i < 5; ++i) r.h160[i] = h[i];
    r.tag = endo | (compressed << 8);
    a.found[idx] = r;
  }
}

// ---- staged filter test ---------------------------------------------------------------------------------------
// Probe 0 (bloom.h) runs on every hash.  Its survivors (37 % at the .blf design density) are not finished on the
// spot - the live lanes would drag all 64 lanes of the wave through up to 19 more dependent probes (measured: 6 % of
// the kernel) - but parked in per-wave rings in LDS and finished 64 at a time (cand_queues below).  Wave-private:
// no barrier, no atomics; records: key offset, hash160, tag.
#define ECL_Q_SLOTS 128u
struct cand_queue {
  u32* mem;    // this wave's slice of LDS: 8 fields x ECL_Q_SLOTS words, field-major (conflict-free for lane-contiguous slots)
  u32 head;    // wave-uniform
  u32 count;   // wave-uniform, < 64 between calls
};

struct cand_rec {
  u64 off;
  u32 h[5], tag;
};
__device__ __forceinline__ cand_rec cand_load(const cand_queue& q, u32 slot) {
  cand_rec r;
  r.off = (u64)q.mem[slot] | (u64)q.mem[ECL_Q_SLOTS + slot] << 32;
#pragma unroll
  for (int i = 0; i < 5; ++i) r.h[i] = q.mem[(2 + i) * ECL_Q_SLOTS + slot];
  r.tag = q.mem[7 * ECL_Q_SLOTS + slot];
  return r;
}
// append the records of the lanes with `pass` (ballot + mbcnt compaction); returns true when 64 or more are waiting.
// Must be reached by ALL lanes of the wave together (head / count are wave-uniform state).
__device__ __forceinline__ bool cand_append(cand_queue& q, bool pass, u64 off, const u32 h[5], u32 tag) {
  const u64 m = __builtin_amdgcn_ballot_w64(pass);
  if (m == 0) return false;
  if (pass) {
    const u32 below = __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
    const u32 slot = (q.head + q.count + below) & (ECL_Q_SLOTS - 1);
    q.mem[slot] = (u32)off;
    q.mem[ECL_Q_SLOTS + slot] = (u32)(off >> 32);
#pragma unroll
    for (int i = 0; i < 5; ++i) q.mem[(2 + i) * ECL_Q_SLOTS + slot] = h[i];
    q.mem[7 * ECL_Q_SLOTS + slot] = tag;
  }
  q.count += (u32)__builtin_popcountll(m);
  return q.count >= 64;
}
// take up to 64 records off the ring: lane i gets record i (valid for i < n)
__device__ __forceinline__ cand_rec cand_take(cand_queue& q, bool& valid) {
  const u32 lane = threadIdx.x & 63u;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const u32 n = q.count < 64 ? q.count : 64;
  valid = lane < n;
  cand_rec r = cand_load(q, (q.head + lane) & (ECL_Q_SLOTS - 1));
  q.head = (q.head + n) & (ECL_Q_SLOTS - 1);
  q.count -= n;
  return r;
}
// the two rings of a wave: A = survivors of probe 0 (37 % of all hashes at the .blf design density), B = survivors of
// the middle stage (probes 1-2: 14 % of A; one probe for multi-GB filters: 37 %).  A is drained 64 at a time without
// a loop; only B runs the remaining probes with the early-out loop, where the wave iterates until its slowest lane
// is done.  Per hash and wave: 68 VALU instructions for the whole filter test instead of 96 with one ring.
// keys: the keys of the call that this wave has brought to check_point (live lanes), wave-uniform, so it lives in SGPRs: per key a bit
// count of the compare mask the range test already produced and a 64-bit add, on the scalar unit.  keys_flush hands it to the call's
// counter at the end of the wave; the host compares the sum with the keys it asked for (ECL_E_COVERAGE)
struct cand_queues {
  cand_queue a, b;
  u64 keys;
};
__device__ __forceinline__ void keys_count(cand_queues& q, bool live) { q.keys += (u64)__builtin_popcountll(__builtin_amdgcn_ballot_w64(live)); }
// one vector atomic per wave and launch (lane 0; every lane of the wave reaches the end of both kernels)
__device__ __forceinline__ void keys_flush(const add_args& a, const cand_queues& q) {
  if ((threadIdx.x & 63u) == 0) atomicAdd(a.keys, (unsigned long long)q.keys);
}
// P2SH: the kernel reports the address type 2 as well, so the type byte of a parked record keeps two bits instead of one (the ETH
// kernels, type 3, instantiate these with P2SH = true for the same reason)
template <bool P2SH>
__device__ __forceinline__ void cand_finish(const add_args& a, cand_queue& qb) {  // up to 64 records of ring B
  bool valid;
  const cand_rec r = cand_take(qb, valid);
  const int from = bloom_mid_two(a.bloom) ? 3 : 2;  // probe 0 and the middle stage's one or two are done
  if (valid && bloom_probes_from(a.bloom, r.h, from))
    found_push(a, r.off, r.h, r.tag & 0xff, (r.tag >> 8) & (P2SH ? 3 : 1));
}
template <bool P2SH>
__device__ __forceinline__ void cand_mid(const add_args& a, cand_queues& q) {  // up to 64 records of ring A -> ring B
  bool valid;
  const cand_rec r = cand_take(q.a, valid);
  const bool pass = valid && bloom_mid(a.bloom, r.h, bloom_mid_two(a.bloom));
  if (cand_append(q.b, pass, r.off, r.h, r.tag)) cand_finish<P2SH>(a, q.b);
}
template <bool P2SH>
__device__ __forceinline__ void cand_push(const add_args& a, cand_queues* q, bool pass, u64 off, const u32 h[5], u32 tag) {
  if (cand_append(q->a, pass, off, h, tag)) cand_mid<P2SH>(a, *q);
}
template <bool P2SH>
__device__ __forceinline__ void cand_flush(const add_args& a, cand_queues& q) {  // end of the kernel: the remainders
  cand_mid<P2SH>(a, q);  // A holds < 64
  cand_finish<P2SH>(a, q.b);  // B holds < 128: at most two rounds
  cand_finish<P2SH>(a, q.b);
}
// Filter test of one hash; q == nullptr: no queue (`mul` kernel), everything in place.  With a queue the call must
// be reached by ALL lanes of the wave together: lanes whose key is outside the range come along with live = false.
// (Deferring the stage-1 test by one hash - loads in flight under the next hash160 - was measured: no gain, the
// other waves of the SIMD already cover the probe latency.)
// ---- the prefix kernels' filter (prefix.h): stage 1 is one bitmap load; its survivors wait in ring A alone and take the exact test 64 at
// a time (one ring is enough: there is no middle stage to thin them out, the exact test either pushes the record or drops it).  The type
// field keeps two bits (ETH is type 3).
__device__ __forceinline__ void prefix_finish(const add_args& a, cand_queue& qa) {
  bool valid;
  const cand_rec r = cand_take(qa, valid);
  if (valid && prefix_exact(a.prefix, r.h)) found_push(a, r.off, r.h, r.tag & 0xff, (r.tag >> 8) & 3);
}
__device__ __forceinline__ void prefix_flush(const add_args& a, cand_queues& q) { prefix_finish(a, q.a); }  // A holds < 64
// ---- the mask kernels' filter (mask.h): the test is exact on the spot, so ring A alone parks the records - it is there so that found_push
// (an atomic and a 32-byte store under divergence) stays out of the per-key loop - and is drained 64 at a time and at the end.  One record
// per (key, image) however many entries match: mask_has answers once.
__device__ __forceinline__ void mask_finish(const add_args& a, cand_queue& qa) {
  bool valid;
  const cand_rec r = cand_take(qa, valid);
  if (valid) found_push(a, r.off, r.h, r.tag & 0xff, (r.tag >> 8) & 3);
}
__device__ __forceinline__ void mask_flush(const add_args& a, cand_queues& q) { mask_finish(a, q.a); }  // A holds < 64
// PREFIX: 0 the bloom, 1 the prefix filter, 2 the mask filter
template <bool P2SH, int PREFIX = 0>
__device__ __forceinline__ void filter_check(const add_args& a, cand_queues* q, bool live, u64 off, const u32 h[5], u32 endo,
                                             u32 compressed) {
  if (PREFIX == 2) {
    const bool in = live && mask_has(a.mask, h);
    if (cand_append(q->a, in, off, h, endo | (compressed << 8))) mask_finish(a, q->a);
    return;
  }
  if (PREFIX == 1) {
    const bool in = live && prefix_stage1(a.prefix, h);
    if (cand_append(q->a, in, off, h, endo | (compressed << 8))) prefix_finish(a, q->a);
    return;
  }
  const bool pass = live && bloom_stage1(a.bloom, h);
  if (!q) {
    if (pass && bloom_stage2(a.bloom, h)) found_push(a, off, h, endo, compressed);
    return;
  }
  cand_push<P2SH>(a, q, pass, off, h, endo | (compressed << 8));
}

// hash every selected encoding / endomorphism image of the affine point (x, y) and probe the filter
// (check_found_add, main.c:287-347; endo images (x,-y) (bx,y) (bx,-y) (b2x,y) (b2x,-y), main.c:314-327).
// P2SH (no reference counterpart): the script hash of the compressed key's hash160, one more SHA-256 and RIPEMD-160 block fed
// by the addr33 hash, which is computed for it even when addr33 itself is not searched.
// ETH (no reference counterpart, searched alone: A33 = A65 = P2SH = false): the Ethereum address of the point, Keccak-256 over x || y
// (keccak.h), type 3; x and y are normalised and the endomorphism images formed as for addr65.
// x: magnitude <= 4, y: magnitude <= 3.
template <bool A33, bool A65, bool P2SH, bool ENDO, bool ETH = false, int PREFIX = 0>
__device__ __forceinline__ void check_point(const add_args& a, cand_queues* q, bool live, fe x, fe y, u64 off) {
  u32 xw[3][8], yw[2][8], par = 0;
  if (ENDO) {
    const u32 bw[8] = FE_BETA1_W;
    fe bx = fe_mul(x, fe_from_words(bw));  // magnitude 1
    fe b2x = fe_neg(fe_add(x, bx), 5);     // beta^2 = -1 - beta; magnitude 6
    fe_normalize(bx);
    fe_normalize(b2x);
    fe_to_words(xw[1], bx);
    fe_to_words(xw[2], b2x);
  }
  fe_normalize(x);
  fe_to_words(xw[0], x);
  if (A65 || ETH) {
    fe_normalize(y);
    fe_to_words(yw[0], y);
    par = y.n[0] & 1u;
    if (ENDO && !ETH) {
      fe ny = fe_neg(y, 1);  // y != 0 on the curve, so this is p - y after normalisation
      fe_normalize(ny);
      fe_to_words(yw[1], ny);
    }
  } else {
    par = fe_parity(y);
  }
  const int nvar = ENDO ? 6 : 1;
#pragma unroll 1
  for (int e = 0; e < nvar; ++e) {
    u32 xs[8], h[5];
#pragma unroll
    for (int i = 0; i < 8; ++i) xs[i] = ENDO ? (e < 2 ? xw[0][i] : (e < 4 ? xw[1][i] : xw[2][i])) : xw[0][i];
    if (A33 || P2SH) {
      hash160_33(h, xs, (par ^ (u32)e) & 1u);  // parity(-y) = !parity(y): p is odd, y != 0
      if (A33) filter_check<P2SH, PREFIX>(a, q, live, off, h, e, 1);
      if (P2SH) {
        u32 hs[5];
        hash160_p2sh(hs, h);
        filter_check<P2SH>(a, q, live, off, hs, e, 2);
      }
    }
    if (A65) {
      u32 ys[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) ys[i] = (ENDO && (e & 1)) ? yw[1][i] : yw[0][i];
      hash160_65(h, xs, ys);
      filter_check<P2SH, PREFIX>(a, q, live, off, h, e, 0);
    }
    if (ETH) {
      u32 ys[8];
      if (ENDO) {
        // -y is formed here, per image, from y's words: p - y = ~y + (p + 1) (mod 2^256), under a mask made of the image number, so
        // that it cannot be hoisted out of the loop - kept for the loop's length as addr65 keeps it, its eight words (beside Keccak's
        // fifty-word state) pushed the walk's values into scratch inside the table loop.  16 instructions per address.
        const u32 m = 0u - ((u32)e & 1u);
        const u32 p1[8] = {0xFFFFFC30u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        u64 c = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          c += (u64)(yw[0][i] ^ m) + (p1[i] & m);
          ys[i] = (u32)c;
          c >>= 32;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) ys[i] = yw[0][i];
      }
      eth_address(h, xs, ys);
      filter_check<true, PREFIX>(a, q, live, off, h, e, 3);
    }
  }
}

// The exact way to the parity of y3 for the addr33-only walk kernels, where emit33_ypar_short's guard fires (2^-16 per key, so a wave
// comes here once in about 2^10 walked points): the step of add_walk.inc once more - lam = (+-Gy - Y) invk, x3 = lam^2 - X - Gx,
// y3 = lam (X - x3) - Y - from values the table loop keeps in any case, so that nothing of the step stays live across the short product
// for this block's sake (kept, lam and X - x3 cost 63 scratch instructions in it).  Out of line: inlined, its 261 multiply-adds sit in
// the `which` loop as a block of 500 instructions that is next to never run.  The caller hands over COPIES made where it calls
// (walk_ypar_copy): arguments by reference are stack objects, and those of X, Y and invk themselves are written where the values are
// made - in the table loop, for every key.
__device__ __forceinline__ fe walk_ypar_copy(const fe& a) {
  fe r = a;
#pragma unroll
  for (int l = 0; l < FE_LIMBS; ++l) asm volatile("" : "+v"(r.n[l]));
  return r;
}
// the step itself, from its numerator s = +-Gy - Y: x3 = lam^2 + nxg with lam = s invk, and the parity of lam (X - x3) - Y.  Both forms
// of the exact way run this and nothing else: walk_ypar_exact below, and the block that add_walk.inc keeps in place with the endomorphism
__device__ __forceinline__ u32 walk_ypar_step(fe& x3, const fe& s, const fe& invk, const fe& nxg, const fe& X, const fe& Y) {
  const fe lam = fe_mul(s, invk);
  x3 = fe_add(fe_sqr(lam), nxg);                                          // magnitude 4
  return fe_parity(fe_sub(fe_mul(lam, fe_add(X, fe_neg(x3, 4))), Y));     // X - x3: magnitude 6; y3: magnitude 3
}
__device__ __noinline__ inline u32 walk_ypar_exact(ctab_ptr gxy, int which, const fe& X, const fe& Y, const fe& invk) {
  const fe gx = fe_ld_tab(gxy), gy = fe_ld_tab(gxy + FE_LIMBS);
  const fe c = which == 0 ? fe_add(gy, fe_neg(fe_zero(), 1)) : fe_neg(gy, 2);
  fe s, x3;
#pragma unroll
  for (int l = 0; l < FE_LIMBS; ++l) s.n[l] = c.n[l] - Y.n[l];
  return walk_ypar_step(x3, s, invk, fe_neg(fe_add(X, gx), 2), X, Y);
}

// check_point<true, false, false, ENDO> for the walk kernels (k_add<true, false, ENDO>): the same hashes, probes and records by emit33.h's
// shorter way - limbs to message words, y for its parity alone, probe 0 from RIPEMD-160's native words, the h160_t byte order only for
// what is parked.  ENDO: the images in check_point's numbering.  x: magnitude <= 4, par: the parity of y's canonical residue (emit33_parity
// of the centre's y, emit33_ypar for a walked point, whose y is never formed).
template <bool ENDO>
__device__ __forceinline__ void check_point33(const add_args& a, cand_queues* q, bool live, const fe& x, u32 par, u64 off) {
  u32 xw[ENDO ? 3 : 1][9];
  if (ENDO) {
    const u32 bw[8] = FE_BETA1_W;
    const fe bx = fe_mul(x, fe_from_words(bw));  // magnitude 1
    const fe b2x = fe_neg(fe_add(x, bx), 5);     // beta^2 = -1 - beta; magnitude 6
    emit33_xwords(xw[1], bx);
    emit33_xwords(xw[ENDO ? 2 : 0], b2x);
  }
  emit33_xwords(xw[0], x);
  const int nvar = ENDO ? 6 : 1;
#pragma unroll 1
  for (int e = 0; e < nvar; ++e) {
    u32 w[9], o[5], h[5];
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = ENDO ? (e < 2 ? xw[0][i] : (e < 4 ? xw[1][i] : xw[ENDO ? 2 : 0][i])) : xw[0][i];
    w[0] |= (0x02u | ((par ^ (u32)e) & 1u)) << 24;  // parity(-y) = !parity(y): p is odd, y != 0
    emit33_hash(o, w);
    const bool pass = live && emit33_probe0(a.bloom, o);
    emit33_h160(h, o);
    cand_push<false>(a, q, pass, off, h, (u32)e | (1u << 8));
  }
}

// ---- Taproot (BIP341 / BIP86 key path), stage A: what the emit kernels (k_add_tr, k_mul_points_tr) do with a point instead of hashing
// and probing it.  The output key of P is the x of a SECOND point, Q = P' + t G with P' the even-y lift of P and t = taptweak(P.x), so a
// key costs a fixed-base scalar multiplication: the point's entry - t (8 words, the layout of a `mul` scalar), P'.x, P'.y (canonical
// words) - goes to a slab in HBM at the key's offset, and k_tr_check (tr_kernels.h) runs `mul`'s machinery over the slab.  96 bytes per
// key, written as six 16-byte stores.  P'.y is even, so bit 0 of its first word is free: it carries the launch's epoch (0 / 1, the host
// alternates it), by which stage B tells an entry of this launch from what an earlier one left there.  isinf (a `mul` scalar that is
// 0 mod n): the entry is x = y = 0, which is no point - stage B counts it as a key without an output.
#define TR_SLAB_WORDS 24u
__device__ __forceinline__ void tr_emit(const add_args& a, bool have, bool isinf, fe x, fe y, u64 off) {
  fe_normalize(x);
  fe_normalize(y);
  u32 xw[8], yw[8], t[8];
  fe_to_words(xw, x);
  fe_to_words(yw, y);
#pragma unroll
  for (int i = 0; i < 8; ++i) xw[i] = isinf ? 0u : xw[i], yw[i] = isinf ? 0u : yw[i];
  tr_lift_y(yw);
  taptweak(t, xw);
  if (have) {
    uint4* e = (uint4*)(a.slab + (size_t)off * TR_SLAB_WORDS);
    e[0] = make_uint4(t[0], t[1], t[2], t[3]), e[1] = make_uint4(t[4], t[5], t[6], t[7]);
    e[2] = make_uint4(xw[0], xw[1], xw[2], xw[3]), e[3] = make_uint4(xw[4], xw[5], xw[6], xw[7]);
    e[4] = make_uint4(yw[0] | a.epoch, yw[1], yw[2], yw[3]), e[5] = make_uint4(yw[4], yw[5], yw[6], yw[7]);
  }
}
// the candidate rings for a kernel that reports ONE address type (k_tr_check: type 4, the public-key kernels: type 5, which the two bits
// the rings keep for the type of the other kernels do not hold): the type is a constant of the kernel.  TAG = false (k_tr_check): the
// ring's tag is not read; TAG = true: it carries the record's endo field (the image number of a public key searched with the endomorphism)
template <u32 TYPE, bool TAG = false>
__device__ __forceinline__ void cand1_finish(const add_args& a, cand_queue& qb) {
  bool valid;
  const cand_rec r = cand_take(qb, valid);
  const int from = bloom_mid_two(a.bloom) ? 3 : 2;
  if (valid && bloom_probes_from(a.bloom, r.h, from)) found_push(a, r.off, r.h, TAG ? r.tag & 0xffu : 0u, TYPE);
}
template <u32 TYPE, bool TAG = false>
__device__ __forceinline__ void cand1_mid(const add_args& a, cand_queues& q) {
  bool valid;
  const cand_rec r = cand_take(q.a, valid);
  const bool pass = valid && bloom_mid(a.bloom, r.h, bloom_mid_two(a.bloom));
  if (cand_append(q.b, pass, r.off, r.h, TAG ? r.tag : 0u)) cand1_finish<TYPE, TAG>(a, q.b);
}
template <u32 TYPE, bool TAG = false>
__device__ __forceinline__ void cand1_check(const add_args& a, cand_queues& q, bool live, u64 off, const u32 h[5], u32 tag = 0) {
  const bool pass = live && bloom_stage1(a.bloom, h);
  if (cand_append(q.a, pass, off, h, TAG ? tag : 0u)) cand1_mid<TYPE, TAG>(a, q);
}
template <u32 TYPE, bool TAG = false>
__device__ __forceinline__ void cand1_flush(const add_args& a, cand_queues& q) {
  cand1_mid<TYPE, TAG>(a, q);
  cand1_finish<TYPE, TAG>(a, q.b);
  cand1_finish<TYPE, TAG>(a, q.b);
}
// ---- public keys by x (-a x, pub_emit.h): what the public-key kernels (k_add_pub<ENDO>, k_mul_check_pub) do with a point's x instead of
// hashing it: the leading 20 bytes of the canonical x through the rings, record type 5.  ENDO: beta x and beta^2 x too, as the +y images
// 0, 2, 4 of check_point's numbering (a key and its negative share x, so three probes stand for six keys and the host's calc_priv
// needs no new case).  x: magnitude <= 4.
template <bool ENDO>
__device__ __forceinline__ void pub_check(const add_args& a, cand_queues& q, bool live, const fe& x, u64 off) {
  u32 h[ENDO ? 3 : 1][5];
  if (ENDO) {
    fe bx, b2x;
    pub_endo_x(bx, b2x, x);
    pub_words20(h[1], bx);
    pub_words20(h[2], b2x);
  }
  pub_words20(h[0], x);
  if (ENDO) {
#pragma unroll 1
    for (u32 e = 0; e < 3; ++e) {
      u32 hs[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) hs[i] = e == 0 ? h[0][i] : (e == 1 ? h[1][i] : h[ENDO ? 2 : 0][i]);
      cand1_check<5u, true>(a, q, live, off, hs, 2u * e);
    }
  } else {
    cand1_check<5u, true>(a, q, live, off, h[0]);
  }
}

// ---- the baby table of `bsgs` (ECL_INSERT): what k_add_pub_ins does with a point's x instead of probing it - the 20 bits of its leading
// 20 bytes are SET in the resident filter (blf_add; 20 atomic ORs).  Only keys of the call (live): the centres, jump points and the keys of
// a last group beyond nkeys that the walk computes as well leave no bit.  No rings, no records.
__device__ __forceinline__ void pub_insert(const add_args& a, bool live, const fe& x) {
  if (!live) return;
  u64 idx[20];
  pub_insert_idx(idx, x);
  unsigned long long* bits = (unsigned long long*)a.bloom.bits;
#pragma unroll
  for (int p = 0; p < 20; ++p) atomicOr(bits + bloom_mod(a.bloom, idx[p] >> 6), 1ull << (idx[p] & 63));
}

// waves per SIMD the register allocator must leave room for (256-thread blocks: blocks per CU = this value).  Final kernel:
// 2 is 2 % slower, 5 is 0.9 % and 6 is 4.8 % slower, 4 is 0.2-0.5 % faster than 3 except for -a cu -endo (0.4 % slower: it
// stays at 3); -a u -endo spills inside its per-point loop at 4 (17 scratch instructions per table point), so it takes 3 as well
#define ECL_ADD_WAVES 4
// threads per workgroup of the add kernel.  Waves never talk to each other (no barrier, wave-private LDS rings), so the
// only thing the size decides is the granularity at which the dispatcher hands out work: 64 / 128 / 256 measured equal
// within 0.1 % in round 2 (tried and rejected); the lane count of a call is a multiple of 256
#define ECL_ADD_BLOCK 256
// The kernel body is written once (add_walk.inc) and instantiated under two names: k_add for addr33 / addr65 and k_add_p2sh for the
// sets that include P2SH.  Two names rather than a fourth template parameter, so that the six instantiations without P2SH keep their
// symbols (tools/isa_mix.py and the tracked profiles/ records are keyed on them); and the body sits in each kernel itself rather than
// in a __device__ function that both call, because the compiler optimises such a function on its own before it inlines it: built
// that way, all six came out with a different register allocation than before (and k_mul_check with 16 more bytes of scratch).
#define ECL_WALK_KERNEL k_add
#define ECL_WALK_P2SH false
#define ECL_WALK_WAVES ((A65 && ENDO) ? 3 : ECL_ADD_WAVES)
#include "add_walk.inc"
#undef ECL_WALK_KERNEL
#undef ECL_WALK_P2SH
#undef ECL_WALK_WAVES
// P2SH instantiations (A33 / A65 = the other types searched with it), at the waves per SIMD of the k_add instantiation with the same
// A65 / ENDO.  All eight keep their per-key loops (prefix products, table, `which`) free of scratch instructions, like the six above:
// what they spill sits in the once-per-group launch loop (tools/isa_mix.py on the built library)
#define ECL_WALK_KERNEL k_add_p2sh
#define ECL_WALK_P2SH true
#define ECL_WALK_WAVES ((A65 && ENDO) ? 3 : ECL_ADD_WAVES)
#include "add_walk.inc"
#undef ECL_WALK_KERNEL
#undef ECL_WALK_P2SH
#undef ECL_WALK_WAVES
// ETH instantiations: k_add_eth<ENDO>, one address type, never combined with the others (ecl_hip_open), so two kernels.  Both at three
// waves per SIMD (168 VGPRs): Keccak's state is 50 registers plus a dozen for the column parities beside the walk's live values, and at
// four waves (128) the plain kernel reloaded the lane's two chain pointers from scratch once per table point; at three it has no spill
// at all, and the -endo kernel spills in the launch loop only (tools/isa_mix.py --eth)
#define ECL_ETH_WAVES 3
#define ECL_WALK_KERNEL k_add_eth
#define ECL_WALK_ETH
#define ECL_WALK_P2SH false
#define ECL_WALK_WAVES ECL_ETH_WAVES
#include "add_walk.inc"
#undef ECL_WALK_KERNEL
#undef ECL_WALK_ETH
#undef ECL_WALK_P2SH
#undef ECL_WALK_WAVES
// Taproot emit instantiation: k_add_tr, the walk with tr_emit in place of the hash-and-probe step (no rings, no filter; it still counts
// the keys it emits).  Taproot is searched alone and without the endomorphism (ecl_hip_open), so one kernel.
#define ECL_TR_WAVES 4
#define ECL_WALK_KERNEL k_add_tr
#define ECL_WALK_TR
#define ECL_WALK_P2SH false
#define ECL_WALK_WAVES ECL_TR_WAVES
#include "add_walk.inc"
#undef ECL_WALK_KERNEL
#undef ECL_WALK_TR
#undef ECL_WALK_P2SH
#undef ECL_WALK_WAVES
// Public-key instantiations: k_add_pub<ENDO>, the walk with x-only emission (pub_emit.h: no y of a walked point, no hash), searched alone
// (ecl_hip_open), so two kernels.  Four waves per SIMD (128 VGPRs, spills in the launch loop only) is the most this kernel can have: five
// cannot be met (the compiler falls back to four: a field multiplication's operands, result and accumulators beside the walk's state do
// not fit 96 VGPRs), and six or eight are out of reach of any register setting - the rings' 32 KiB of LDS per block cap a CU at five
// blocks; asked for, the compiler builds a 159-VGPR kernel that runs at three (HISTORY section 11)
#define ECL_PUB_WAVES 4
#define ECL_WALK_KERNEL k_add_pub
#define ECL_WALK_PUB
#define ECL_WALK_P2SH false
#define ECL_WALK_WAVES ECL_PUB_WAVES
#include "add_walk.inc"
#undef ECL_WALK_KERNEL
#undef ECL_WALK_PUB
#undef ECL_WALK_P2SH
#undef ECL_WALK_WAVES
// Insert instantiation: k_add_pub_ins, the x-only walk with pub_insert in place of pub_check (no rings, no records, no template: the baby
// table of `bsgs` is built without the endomorphism).  It still counts the keys it inserts.
#define ECL_WALK_KERNEL k_add_pub_ins
#define ECL_WALK_PUB
#define ECL_WALK_INSERT
#define ECL_WALK_P2SH false
#define ECL_WALK_WAVES ECL_PUB_WAVES
#include "add_walk.inc"
#undef ECL_WALK_KERNEL
#undef ECL_WALK_PUB
#undef ECL_WALK_INSERT
#undef ECL_WALK_P2SH
#undef ECL_WALK_WAVES
// Prefix instantiations (-p, ECL_PREFIX): k_add_pfx<A33, A65, ENDO> and k_add_pfx_eth<ENDO>, the walk and the hashes of k_add / k_add_eth
// with the prefix filter (prefix.h) in place of the bloom and one ring in place of two; at the waves per SIMD of the kernel they mirror.
#define ECL_WALK_KERNEL k_add_pfx
#define ECL_WALK_PREFIX
#define ECL_WALK_P2SH false
#define ECL_WALK_WAVES ((A65 && ENDO) ? 3 : ECL_ADD_WAVES)
#include "add_walk.inc"
#undef ECL_WALK_KERNEL
#undef ECL_WALK_P2SH
#undef ECL_WALK_WAVES
#define ECL_WALK_KERNEL k_add_pfx_eth
#define ECL_WALK_ETH
#define ECL_WALK_P2SH false
#define ECL_WALK_WAVES ECL_ETH_WAVES
#include "add_walk.inc"
#undef ECL_WALK_KERNEL
#undef ECL_WALK_ETH
#undef ECL_WALK_PREFIX
#undef ECL_WALK_P2SH
#undef ECL_WALK_WAVES
// Mask instantiations (-p 0xdead*beef, ECL_MASK): k_add_msk_eth<ENDO>, the walk and Keccak of k_add_pfx_eth with the mask filter (mask.h) in
// place of the prefix filter; one ring, the waves per SIMD of the kernel they mirror.
#define ECL_WALK_KERNEL k_add_msk_eth
#define ECL_WALK_ETH
#define ECL_WALK_PREFIX
#define ECL_WALK_MASK
#define ECL_WALK_P2SH false
#define ECL_WALK_WAVES ECL_ETH_WAVES
#include "add_walk.inc"
#undef ECL_WALK_KERNEL
#undef ECL_WALK_ETH
#undef ECL_WALK_PREFIX
#undef ECL_WALK_MASK
#undef ECL_WALK_P2SH
#undef ECL_WALK_WAVES
