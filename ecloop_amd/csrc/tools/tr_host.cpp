// tr_host.cpp — compiles the Taproot pieces of the DEVICE headers for the host with g++, so that the CPU test-suite can check them without
// a GPU (tests/test_tr_host.py): the tagged hash, the tweak's range test and the even-y lift of hash160.h, and the XYZZ + affine
// addition of stage B with its out-of-line fallback (ec.h: xyzz_madd_lazy, then jac_madd where ZZ = 0, as k_tr_check does).
// Not part of the product library.
#include "../hash160.h"
#include "../ec.h"
#include <stddef.h>

extern "C" {
// t[i] = taptweak(x[i]) (8 little-endian words each), ge[i] = t[i] >= n
void th_tweak_many(const u32* xw, u32* tw, unsigned char* ge, u32 n) {
  for (u32 i = 0; i < n; ++i) {
    taptweak(tw + (size_t)i * 8, xw + (size_t)i * 8);
    ge[i] = tr_tweak_ge_n(tw + (size_t)i * 8);
  }
}
void th_ge_n_many(const u32* tw, unsigned char* ge, u32 n) {
  for (u32 i = 0; i < n; ++i) ge[i] = tr_tweak_ge_n(tw + (size_t)i * 8);
}
void th_lift_many(u32* yw, u32 n) {
  for (u32 i = 0; i < n; ++i) tr_lift_y(yw + (size_t)i * 8);
}
// T (affine tx, ty; tinf != 0: the point at infinity) + P' (px, py): the lazy XYZZ addition from T as (X, Y, ZZ = ZZZ = 1), and where it
// leaves ZZ = 0 (or T is infinity) the complete one.  out: x of the sum (8 words); returns 0 for the point at infinity, 1 lazy, 2 complete.
int th_add_x(const u32 tx[8], const u32 ty[8], int tinf, const u32 px[8], const u32 py[8], u32 out[8]) {
  const fe qx = fe_from_words(px), qy = fe_from_words(py);
  jac j;
  j.X = fe_from_words(tx), j.Y = fe_from_words(ty), j.Z = fe_one(), j.inf = tinf ? 1 : 0;
  xyzz a;
  a.X = j.X, a.Y = j.Y, a.ZZ = fe_one(), a.ZZZ = fe_one(), a.inf = 0;
  xyzz r = xyzz_madd_lazy(a, qx, qy);
  int how = 1;
  if (tinf || fe_is_zero(r.ZZ)) r = xyzz_from_jac(jac_madd(j, qx, qy)), how = 2;
  if (r.inf) return 0;
  fe x = fe_mul(r.X, fe_inv(r.ZZ));
  fe_normalize(x);
  fe_to_words(out, x);
  return how;
}
}
