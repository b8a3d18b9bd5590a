// tr_kernels.h - Taproot (BIP341 / BIP86 key path, "bc1p...") on the device, stage B and the verification path.
// (one translation unit: included by ecloop_hip.hip after mul_kernels.h)
//
// The output key of a public key P is Q.x with Q = P' + t G, P' the even-y lift of P and t = taptweak(P.x) (hash160.h): not a hash of
// P but a second point, one fixed-base scalar multiplication per key.  Stage A (tr_emit, add_kernel.h: k_add_tr from the walk,
// k_mul_points_tr from `mul`'s window sums) leaves t and P' of every key in a slab in HBM; stage B below is the body of k_mul_check over
// that slab: t G by wtab_sum_fast on the context's `mul` table, + P' by one more mixed addition, one inversion per thread for all of its
// keys, x = X / ZZ, and the leading 20 bytes of x go through the candidate rings as every other type's hash does (record type 4).
#pragma once
#include "mul_kernels.h"

// t G + P' by the complete formulas, out of line: t = 0 (no digit), t G = +-P' (h = 0 in the last addition) or a sum that degenerated
// on the way.  inf = 1: the key has no output key (t G = -P').
__device__ __noinline__ xyzz tr_sum_complete(const u32* __restrict__ e, const wtab t) {
  u32 kk[9], xw[8], yw[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) kk[j] = e[j], xw[j] = e[8 + j], yw[j] = e[16 + j];
  kk[8] = 0;
  yw[0] &= ~1u;
  return xyzz_from_jac(jac_madd(wtab_sum(kk, t), fe_from_words(xw), fe_from_words(yw)));
}

// keys per thread of k_tr_check at most (one shared inversion; one bit of `nomask` each): a launch covers up to nt * R entries, the host
// walks a slab in launches of what the chip holds at once, as `mul` walks a call in pieces
#define TR_R 12u
// slab: n entries of TR_SLAB_WORDS words (tr_emit); epoch: the mark this launch's entries carry - an entry with the other mark was left by
// an earlier launch (stage A fell short): it is neither tweaked nor counted, and the call fails its coverage check.  Counted (a.keys):
// entries of this epoch, whether they have an output key or not (t >= n, the stand-in of a scalar 0 (mod n), t G = -P').
// base: the call's offset of entry 0.  DIAG (ecl_hip_diag_tr): the whole output key of every entry, 8 big-endian words, and ok_out,
// instead of the filter test.
template <bool DIAG>
__global__ void __launch_bounds__(256, ECL_MUL_WAVES) k_tr_check(const u32* __restrict__ slab, u32 n, u64 base, const wtab gtab, add_args a, u32 epoch,
                                                                 u32* __restrict__ tmp, u32 nt, u32 R, u32* __restrict__ qx_out, u8* __restrict__ ok_out) {
  __shared__ u32 q_mem[4][2][8 * ECL_Q_SLOTS];  // two candidate rings per wave (add_kernel.h)
  const u32 t = blockIdx.x * 256u + threadIdx.x;
  if (t >= nt) return;  // nt is a multiple of 256: whole workgroups leave
  fe prod = fe_one();
  u32 nomask = 0;  // keys without an output key
  u32 stalemask = 0;  // entries that are not of this launch
  // parked per key: X, ZZ and the running product of the ZZ's; x = X / ZZ
#pragma unroll 1
  for (u32 r = 0; r < R; ++r) {
    const u32 i = r * nt + t;
    if (i >= n) break;
    const u32* e = slab + (size_t)i * TR_SLAB_WORDS;
    u32 bad;
    xyzz acc = wtab_sum_fast(e, gtab, bad);
    const uint4 x0 = ((const uint4*)e)[2], x1 = ((const uint4*)e)[3], y0 = ((const uint4*)e)[4], y1 = ((const uint4*)e)[5];
    const u32 xw[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w}, yw[8] = {y0.x & ~1u, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
    acc = xyzz_madd_lazy(acc, fe_from_words(xw), fe_from_words(yw));
    // a zero digit of t, a sum that degenerated on the way, or t G = +-P' in the last addition (h = 0) leave ZZ = 0 - and a zero in
    // the product chain would take the thread's other keys with it: the complete sum, out of line
    if (__builtin_expect(bad || fe_is_zero(acc.ZZ), 0)) acc = tr_sum_complete(e, gtab);
    u32 any = 0, tw[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) any |= xw[j] | yw[j], tw[j] = e[j];
    const bool stale = (y0.x & 1u) != epoch;
    const bool none = stale || acc.inf || any == 0u || tr_tweak_ge_n(tw);
    nomask |= (none ? 1u : 0u) << r, stalemask |= (stale ? 1u : 0u) << r;
    if (none) acc.ZZ = fe_one();
    u32* p = tmp + (size_t)r * 27 * nt + t;
#pragma unroll
    for (int l = 0; l < FE_LIMBS; ++l) p[(size_t)l * nt] = acc.X.n[l], p[(size_t)(9 + l) * nt] = acc.ZZ.n[l], p[(size_t)(18 + l) * nt] = prod.n[l];
    prod = fe_mul(prod, acc.ZZ);
  }
  fe inv = fe_inv(prod);
  // every lane of the wave walks all R rounds (the rings' state is wave-uniform): a lane without a key comes along with live = false
  cand_queues q;
  q.a.mem = q_mem[threadIdx.x >> 6][0], q.a.head = 0, q.a.count = 0;
  q.b.mem = q_mem[threadIdx.x >> 6][1], q.b.head = 0, q.b.count = 0;
  q.keys = 0;
#pragma unroll 1
  for (u32 r = R; r-- > 0;) {
    const u32 i = r * nt + t;
    const bool have = i < n;
    const u32* p = tmp + (size_t)r * 27 * nt + t;
    fe X, ZZ, pre;
#pragma unroll
    for (int l = 0; l < FE_LIMBS; ++l) {
      X.n[l] = have ? p[(size_t)l * nt] : 0u;
      ZZ.n[l] = have ? p[(size_t)(9 + l) * nt] : (l == 0 ? 1u : 0u), pre.n[l] = have ? p[(size_t)(18 + l) * nt] : 0u;
    }
    fe zi, ninv;
    fe_mul_pair(zi, ninv, inv, pre, inv, ZZ);  // ZZ = 1 for a lane without a key in this round
    inv = ninv;
    fe x = fe_mul(X, zi);
    fe_normalize(x);
    u32 xw[8], h[5];
    fe_to_words(xw, x);
#pragma unroll
    for (int j = 0; j < 5; ++j) h[j] = xw[7 - j];  // the leading 20 bytes of x as h160_t words
    const bool live = have && !((nomask >> r) & 1u);
    keys_count(q, have && !((stalemask >> r) & 1u));
    if (DIAG) {
      if (have) {
#pragma unroll
        for (int j = 0; j < 8; ++j) qx_out[(size_t)i * 8 + j] = live ? xw[7 - j] : 0u;
        ok_out[i] = live ? 1 : 0;
      }
    } else {
      cand1_check<4u>(a, q, live, base + i, h);
    }
  }
  if (!DIAG) cand1_flush<4u>(a, q);
  keys_flush(a, q);
}

// stage A for n affine points given by the caller (ecl_hip_diag_tr): tr_emit, the function of the emit kernels, one lane per point
__global__ void __launch_bounds__(64) k_tr_emit_points(const u32* __restrict__ x, const u32* __restrict__ y, u32 n, add_args a) {
  const u32 i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  tr_emit(a, true, false, fe_ldw(x + (size_t)i * 8), fe_ldw(y + (size_t)i * 8), i);
}

// the Taproot half of pk_verify_hash (ecl_hip_verify_tr): the output key of each private key by ecl_hip_verify's path - the W = 14 window
// table and an inversion of its own, for k G and again for t G + P' - which shares nothing with the search kernels but the tagged hash.
// qx: 8 big-endian words per key; ok = 0: k = 0 (mod n), t >= n or Q at infinity.
__global__ void __launch_bounds__(64) k_verify_tr(const u32* __restrict__ k, u32 n, const u32* __restrict__ gtab, u32* __restrict__ qx, u8* __restrict__ ok) {
  const u32 i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  u32 kk[9];
#pragma unroll
  for (int w = 0; w < 8; ++w) kk[w] = k[(size_t)i * 8 + w];
  kk[8] = 0;
  fe x, y;
  int fin = jac_to_affine(x, y, gtable_mul(kk, gtab));
  u32 xw[8], yw[8], tw[9];
  fe_to_words(xw, x), fe_to_words(yw, y);
  tr_lift_y(yw);
  taptweak(tw, xw);
  tw[8] = 0;
  if (tr_tweak_ge_n(tw)) fin = 0;
  fe qxe, qye;
  if (fin) fin = jac_to_affine(qxe, qye, jac_madd(gtable_mul(tw, gtab), fe_from_words(xw), fe_from_words(yw)));
  u32 qw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (fin) fe_to_words(qw, qxe);
#pragma unroll
  for (int w = 0; w < 8; ++w) qx[(size_t)i * 8 + w] = qw[7 - w];
  ok[i] = (u8)fin;
}
