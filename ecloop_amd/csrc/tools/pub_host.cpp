// pub_host.cpp — compiles the public-key pieces of the DEVICE headers (pub_emit.h) for the host with g++, so that the CPU test-suite can
// check them without a GPU (tests/test_pub_host.py): the x-only pair step of the walk, the x of the endomorphism images and the 20 bytes
// that are probed.  Not part of the product library.
#include "../pub_emit.h"
#include <stddef.h>

extern "C" {
// per item: the centre (X, Y), a table point (gx, gy) - 8 canonical little-endian words each - -> the x of C + G and of C - G by
// pub_pair_x with invk = 1 / (gx - X) formed as the walk forms it (a weakly normalised difference through fe_inv), 8 words each
void ph_pair_many(const u32* X, const u32* Y, const u32* gx, const u32* gy, u32* xp, u32* xm, u32 n) {
  for (u32 i = 0; i < n; ++i) {
    const fe cx = fe_from_words(X + (size_t)i * 8), cy = fe_from_words(Y + (size_t)i * 8);
    const fe tx = fe_from_words(gx + (size_t)i * 8), ty = fe_from_words(gy + (size_t)i * 8);
    fe d = fe_sub(tx, cx);
    fe_normalize_weak(d);
    const fe invk = fe_inv(d);
    fe a, b;
    pub_pair_x(a, b, cx, cy, tx, ty, invk);
    fe_normalize(a), fe_normalize(b);
    fe_to_words(xp + (size_t)i * 8, a), fe_to_words(xm + (size_t)i * 8, b);
  }
}
// per item: x (8 canonical words), lifted to magnitude `mag` (1 ... 4: x + (mag - 1) p, the form a walked x arrives in) -> the five probed
// words of x, beta x and beta^2 x (15 words)
void ph_probe_many(const u32* x, u32 mag, u32* h, u32 n) {
  for (u32 i = 0; i < n; ++i) {
    fe v = fe_from_words(x + (size_t)i * 8);
    for (u32 m = 1; m < mag; ++m) v = fe_add(v, fe_neg(fe_zero(), 0));  // + p
    fe bx, b2x;
    pub_endo_x(bx, b2x, v);
    pub_words20(h + (size_t)i * 15, v), pub_words20(h + (size_t)i * 15 + 5, bx), pub_words20(h + (size_t)i * 15 + 10, b2x);
  }
}
}
