// herd_kernel.h — the `kangaroo` hot loop on gfx950: a herd of pseudo-random walks (Pollard's lambda method), many kangaroos per lane.
// (ECL_PUB | ECL_HERD; the method is defined in host/kangaroo_plan.h, the host side is abi_herd.h)
//
// Every other kernel of the project walks an arithmetic progression around a lane centre, so all lanes add the SAME table point.  Here
// each kangaroo picks its own table point from its own x, so the table operand is per lane.  What is kept from the add kernel is the
// shared inversion with its prefix products parked in HBM (add_walk.inc); what is new:
//   * one lane owns HERD_M kangaroos (kangaroo i belongs to lane i mod L, slot i / L, L = ceil(H / HERD_M) lanes), the state - x, y as
//     9x29 limbs, the 128-bit distance - lives in HBM as a structure of arrays indexed by i, so a wave's loads and stores of one slot are
//     contiguous; slots with i >= H are masked (a herd of 2 is one lane with two of its slots in use);
//   * a step of a lane: pass 1 over its kangaroos (load x, pick j, T_j.x - x into the running product, park the prefix), ONE fe_inv, pass 2
//     backwards (recover 1 / (T_j.x - x), lambda, the new x and y, the distance; x is made canonical once: it is the next step's j, the
//     distinguished-point test and the record's identity);
//   * the 32 x (x, y, s) jump table sits in LDS, limb-major ([limb][j]: lanes with different j read different banks, equal j broadcast);
//   * a launch loops over steps inside the kernel; the host caps the steps of a launch;
//   * a distinguished point is a record behind an atomicAdd on the call's counter, written with ordinary vector stores.
// The step arithmetic below is __host__ __device__: csrc/tools/kangaroo_host.cpp compiles it with g++ for the CPU tests.
#pragma once
#include "fe256.h"

#define HERD_M 32u            /* kangaroos per lane: DESIGN.md section 7 (f10) has the counts behind the choice */
#define HERD_BLOCK 64         /* threads per workgroup: one wave; waves share nothing but the table */
#define HERD_WAVES 4          /* waves per SIMD the register allocator leaves room for (128 VGPRs) */
#define HERD_TAB_LIMBS 22u    /* table rows: x limbs 0..8, y limbs 9..17, the distance's four words 18..21; row-major [row][j] */
#define HERD_TAB_WORDS (HERD_TAB_LIMBS * 32u)
#define HERD_TAB_IN 20u       /* the table as the host uploads it: per entry x[8], y[8] (canonical words), s[4] */
#define HERD_TYPE 6u          /* ecl_found.compressed of a distinguished point (label dp) */

// ---- the step arithmetic (host and device) -----------------------------------------------------------------------------------
// j of a canonical x: bits 32..36 (limb 1 holds bits 29..57)
FE_FN u32 herd_pick(const fe& x) { return (x.n[1] >> 3) & 31u; }
FE_FN bool herd_same_x(const fe& a, const fe& b) {  // both canonical
  u32 d = 0;
#pragma unroll
  for (int l = 0; l < FE_LIMBS; ++l) d |= a.n[l] ^ b.n[l];
  return d == 0;
}
FE_FN fe herd_tab_fe(const u32* tab, u32 row, u32 j) {
  fe r;
#pragma unroll
  for (int l = 0; l < FE_LIMBS; ++l) r.n[l] = tab[(row + l) * 32u + j];
  return r;
}
// the table entry of this jump and its x: j of x, or j + 1 mod 32 where T_j has the kangaroo's x (the sum would be a doubling or the point at
// infinity; T_j and T_j+1 differ in x, so the difference the shared inversion sees is never zero)
FE_FN u32 herd_jump_index(const u32* tab, const fe& x, fe& tx) {
  u32 j = herd_pick(x);
  tx = herd_tab_fe(tab, 0, j);
  if (herd_same_x(tx, x)) {
    j = (j + 1u) & 31u;
    tx = herd_tab_fe(tab, 0, j);
  }
  return j;
}
// (x, y) + (tx, ty) given invk = 1 / (tx - x): x canonical out, y magnitude 1.  x canonical, y magnitude 1, table normalised.
FE_FN void herd_add(fe& x, fe& y, const fe& tx, const fe& ty, const fe& invk) {
  const fe lam = fe_mul(fe_sub(ty, y), invk);                  // ty - y: magnitude 3
  fe x3 = fe_add(fe_sqr(lam), fe_neg(fe_add(x, tx), 2));       // magnitude 4
  fe y3 = fe_sub(fe_mul(lam, fe_add(x, fe_neg(x3, 4))), y);    // x - x3: magnitude 6; y3: magnitude 3
  fe_normalize(x3);
  fe_normalize_weak(y3);
  x = x3, y = y3;
}
// d += s on four 32-bit words; returns the carry out of 2^128
FE_FN u32 herd_dist_add(u32 d[4], const u32 s[4]) {
  u64 c = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    c += (u64)d[w] + s[w];
    d[w] = (u32)c;
    c >>= 32;
  }
  return (u32)c;
}
// one jump of one kangaroo with table entry j (x of it: tx) and invk = 1 / (tx - x); returns the distance's carry
FE_FN u32 herd_jump(fe& x, fe& y, u32 d[4], const u32* tab, u32 j, const fe& tx, const fe& invk) {
  herd_add(x, y, tx, herd_tab_fe(tab, 9, j), invk);
  u32 s[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) s[w] = tab[(18u + w) * 32u + j];
  return herd_dist_add(d, s);
}
// distinguished: the low dp bits of the canonical x are zero (mask = 2^dp - 1, dp <= 32)
FE_FN bool herd_is_dp(const fe& x, u32 mask) { return ((x.n[0] | (x.n[1] << 29)) & mask) == 0; }
// the record of a distinguished point as the eight words of an ecl_found_dev: key_offset = distance bits 0..63, h160[0], [1] = distance
// bits 96..127, 64..95, h160[2..4] = the leading 12 bytes of x (h160_t's word order), tag = herd (0 tame, 1 wild) | type 6 << 8
FE_FN void herd_record(u32 rec[8], u32 i, const u32 d[4], const fe& x) {
  u32 w[8];
  fe_to_words(w, x);
  rec[0] = d[0], rec[1] = d[1], rec[2] = d[3], rec[3] = d[2];
  rec[4] = w[7], rec[5] = w[6], rec[6] = w[5];
  rec[7] = (i & 1u) | (HERD_TYPE << 8);
}
// the table in its working layout from the uploaded one (entry j: x[8], y[8], s[4]); `part` 0: x and s, 1: y
FE_FN void herd_tab_fill(u32* tab, const u32* in, u32 j, u32 part) {
  u32 w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = in[j * HERD_TAB_IN + part * 8u + k];
  const fe v = fe_from_words(w);
#pragma unroll
  for (int l = 0; l < FE_LIMBS; ++l) tab[(part * 9u + l) * 32u + j] = v.n[l];
  if (!part) {
#pragma unroll
    for (int k = 0; k < 4; ++k) tab[(18u + k) * 32u + j] = in[j * HERD_TAB_IN + 16u + k];
  }
}

#ifdef __HIPCC__
// ---- the kernels ------------------------------------------------------------------------------------------------------------
struct herd_args {
  const u32* __restrict__ tab;   // [32][HERD_TAB_IN]
  u32* __restrict__ state;       // 22 H words: x limbs 0..7 as two uint4 planes of H, y the same, the distance as one uint4 plane, then x limb 8, y limb 8
  uint4* __restrict__ scratch;   // prefix products, the layout of add_kernel.h: [(m * 2 + half) * T + lane]
  u32* __restrict__ scratch2;    // [m * T + lane]
  uint4* __restrict__ found;     // records (ecl_found_dev as two uint4)
  u32* __restrict__ counter;     // [0] records; [6] flags: bit 0 a distance passed 2^128, bit 1 a start was the point at infinity
  unsigned long long* __restrict__ jumps;  // the call's jump count
  u32 cap;
  u32 H, L, T;                   // kangaroos, lanes that own some, threads launched (the scratch planes' stride)
  u32 steps;                     // jumps per kangaroo in this launch
  u32 dpmask;
};

__global__ void __launch_bounds__(HERD_BLOCK, HERD_WAVES) k_herd_walk(const herd_args a) {
  __shared__ u32 tab[HERD_TAB_WORDS];
  herd_tab_fill(tab, a.tab, threadIdx.x & 31u, threadIdx.x >> 5);
  __syncthreads();
  const u32 g = blockIdx.x * (u32)HERD_BLOCK + threadIdx.x;
  if (g >= a.L) return;
  const size_t H = a.H, plane = a.T, s4 = 2 * (size_t)a.T;
  uint4* const X4 = (uint4*)a.state;
  uint4* const Y4 = X4 + 2 * H;
  uint4* const D4 = Y4 + 2 * H;
  u32* const X1 = (u32*)(D4 + H);
  u32* const Y1 = X1 + H;
  uint4* const scr4 = a.scratch + g;
  u32* const scr2 = a.scratch2 + g;
  unsigned long long made = 0;
  u32 over = 0;
#pragma unroll 1
  for (u32 step = 0; step < a.steps; ++step) {
    // ---- pass 1: prefix products of T_j.x - x over the lane's kangaroos (differences have magnitude 3)
    fe acc = fe_one();
#pragma unroll 1
    for (u32 m = 0; m < HERD_M; ++m) {
      const size_t i = (size_t)m * a.L + g;
      if (i >= H) break;  // slots only grow in i
      const fe x = fe_ld_limbs(X4 + i, H, X1 + i);
      fe tx;
      herd_jump_index(tab, x, tx);
      fe_st_limbs(scr4 + (size_t)m * s4, plane, scr2 + (size_t)m * plane, acc);
      acc = fe_mul(acc, fe_sub(tx, x));
    }
    // ---- one inversion for the lane
    fe inv = fe_inv(acc);
    // ---- pass 2, backwards: the jumps
#pragma unroll 1
    for (u32 m = HERD_M; m-- > 0;) {
      const size_t i = (size_t)m * a.L + g;
      if (i >= H) continue;
      const fe pre = fe_ld_limbs(scr4 + (size_t)m * s4, plane, scr2 + (size_t)m * plane);
      fe x = fe_ld_limbs(X4 + i, H, X1 + i), y = fe_ld_limbs(Y4 + i, H, Y1 + i), tx;
      const u32 j = herd_jump_index(tab, x, tx);
      const fe invk = fe_mul(inv, pre);  // 1 / (T_j.x - x)
      inv = fe_mul(inv, fe_sub(tx, x));
      const uint4 dv = D4[i];
      u32 d[4] = {dv.x, dv.y, dv.z, dv.w};
      over |= herd_jump(x, y, d, tab, j, tx, invk);
      fe_st_limbs(X4 + i, H, X1 + i, x);
      fe_st_limbs(Y4 + i, H, Y1 + i, y);
      D4[i] = make_uint4(d[0], d[1], d[2], d[3]);
      ++made;
      if (herd_is_dp(x, a.dpmask)) {
        const u32 idx = atomicAdd(a.counter, 1u);
        if (idx < a.cap) {
          u32 r[8];
          herd_record(r, (u32)i, d, x);
          a.found[2 * (size_t)idx] = make_uint4(r[0], r[1], r[2], r[3]);
          a.found[2 * (size_t)idx + 1] = make_uint4(r[4], r[5], r[6], r[7]);
        }
      }
    }
  }
  atomicAdd(a.jumps, made);
  if (over) atomicOr(a.counter + 6, 1u);
}

// the herd's starts: pts[t] = (B + r_i) G (tame, i even) or r_i G (wild, i odd) from k_mul_g, i = first + t; a wild kangaroo adds Q by the
// complete formulas (r_i = 0: Q itself).  State out: x, y as limbs, the distance r_i.  A start that is the point at infinity sets flag bit 1.
struct herd_q { u32 w[16]; };
__global__ void __launch_bounds__(64) k_herd_init(const u32* __restrict__ pts, const u8* __restrict__ ok, const u32* __restrict__ r, herd_q q,
                                                   u32* __restrict__ state, u32 H, u32 first, u32 n, u32* __restrict__ counter) {
  const u32 t = blockIdx.x * 64u + threadIdx.x;
  if (t >= n) return;
  const size_t i = (size_t)first + t, Hs = H;
  if (i >= Hs) return;
  u32 p[16], qw[16];
#pragma unroll
  for (int w = 0; w < 16; ++w) p[w] = pts[(size_t)t * 16 + w], qw[w] = q.w[w];
  int fin = ok[t];
  if (i & 1u) {
    if (!fin) {
#pragma unroll
      for (int w = 0; w < 16; ++w) p[w] = qw[w];
      fin = 1;
    } else {
      u32 out[16];
#pragma unroll
      for (int w = 0; w < 16; ++w) out[w] = 0;
      fin = ec_add_origin(out, p, qw);
#pragma unroll
      for (int w = 0; w < 16; ++w) p[w] = out[w];
    }
  }
  if (!fin) {
    atomicOr(counter + 6, 2u);
    return;
  }
  uint4* const X4 = (uint4*)state;
  uint4* const Y4 = X4 + 2 * Hs;
  uint4* const D4 = Y4 + 2 * Hs;
  u32* const X1 = (u32*)(D4 + Hs);
  u32* const Y1 = X1 + Hs;
  fe_st_limbs(X4 + i, Hs, X1 + i, fe_from_words(p));
  fe_st_limbs(Y4 + i, Hs, Y1 + i, fe_from_words(p + 8));
  D4[i] = make_uint4(r[(size_t)t * 4], r[(size_t)t * 4 + 1], r[(size_t)t * 4 + 2], r[(size_t)t * 4 + 3]);
}
#endif
