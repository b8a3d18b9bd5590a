// pub_emit.h - public keys searched by their x coordinate (-a x, ECL_PUB): the arithmetic of the x-only walk and what is probed.
// (host and device: tests/test_pub_host.py compiles these with g++ through csrc/tools/pub_host.cpp)
//
// A list of public keys (P2PK outputs, spent-from keys, puzzle keys with a revealed public key) needs no hash: the walk has x in
// registers before any hashing starts.  The y of a walked point is never needed either - C +- G_i has
//   lambda = (+-Gy - Y) / (Gx - X),   x = lambda^2 - (X + Gx)
// and the centre's Y steps on by itself - so a key costs one multiplication and one squaring after its share of invk, against
// 3.5 M + 1 S + hash160.  What is probed: the LEADING 20 BYTES of x as five big-endian words (the word order k_tr_check uses for an
// output key), 160 bits like every other type; the host re-derives a hit and compares all 32.
#pragma once
#include "bloom.h"
#include "fe256.h"

// +-Gy - Y, magnitude 3 (which = 0: C + G_i, 1: C - G_i).  gy: the table's y (normalised), Y: magnitude 1.  `which` is wave-uniform
// in the walk, so the table side (Gy + 2p or 3p - Gy) is selected on the scalar unit and the vector side is one subtraction per limb.
FE_FN fe pub_num(const fe& gy, const fe& Y, int which) {
  const fe c = which == 0 ? fe_add(gy, fe_neg(fe_zero(), 1)) : fe_neg(gy, 2);
  fe s;
#pragma unroll
  for (int l = 0; l < FE_LIMBS; ++l) s.n[l] = c.n[l] - Y.n[l];
  return s;
}
// x of C +- G_i from its numerator, invk = 1 / (Gx - X) and nxg = -(X + Gx) (magnitude 3): magnitude 4
FE_FN fe pub_x(const fe& num, const fe& invk, const fe& nxg) { return fe_add(fe_sqr(fe_mul(num, invk)), nxg); }
// the pair step as a whole (the walk hoists nxg out of its loop over the two signs; the test takes it in one piece)
FE_FN void pub_pair_x(fe& xp, fe& xm, const fe& X, const fe& Y, const fe& gx, const fe& gy, const fe& invk) {
  const fe nxg = fe_neg(fe_add(X, gx), 2);
  xp = pub_x(pub_num(gy, Y, 0), invk, nxg);
  xm = pub_x(pub_num(gy, Y, 1), invk, nxg);
}
// the x of the endomorphism images: beta x (lambda k and its negative) and beta^2 x = -x - beta x (lambda^2 k and its negative).
// x: magnitude <= 4; bx: magnitude 1, b2x: magnitude 6.  A key and its negative share x: three probes cover six keys.
FE_FN void pub_endo_x(fe& bx, fe& b2x, const fe& x) {
  const u32 bw[8] = FE_BETA1_W;
  bx = fe_mul(x, fe_from_words(bw));
  b2x = fe_neg(fe_add(x, bx), 5);
}
// the 160 bits that are probed: the canonical x, its five leading big-endian words (h160_t's word order).  x: magnitude <= 6.
FE_FN void pub_words20(u32 h[5], fe x) {
  fe_normalize(x);
  u32 w[8];
  fe_to_words(w, x);
#pragma unroll
  for (int j = 0; j < 5; ++j) h[j] = w[7 - j];
}
// the baby table of `bsgs` (ECL_INSERT): the 20 bit positions blf_add (bloom.h: bloom_index, lib/utils.c:290-306) gives the 160 probed bits of
// x, before the reduction to the filter's size - what k_add_pub_ins sets and pub_check later probes.  x: magnitude <= 6.
FE_FN void pub_insert_idx(u64 idx[20], const fe& x) {
  u32 h[5];
  u64 a[5];
  pub_words20(h, x);
  bloom_words_of(a, h);
#pragma unroll
  for (int p = 0; p < 20; ++p) idx[p] = bloom_index(a, p);
}
