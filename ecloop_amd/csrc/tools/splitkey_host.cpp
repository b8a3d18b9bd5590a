// splitkey_host.cpp — compiles the arithmetic of the split-key search (host/splitkey.h: the image of an origin, the image of a scalar, the
// requester's combination) for the host with g++, so that the CPU test-suite can check it (tests/test_splitkey_host.py) against Python over
// the oracle's points.  Built as a shared object for the tests; it has a main of its own as well (a self-check over the curve, with the
// double-and-add of ec.h), so the same code can be built as a program under a sanitizer and run directly.  Not part of the product library.
#include "../ec.h"
#include "../../host/splitkey.h"
#include <stdio.h>

static bsgs_int int_of(const uint64_t* w) {
  bsgs_int r;
  memcpy(r.w, w, 32);
  return r;
}

extern "C" {
void sk_host_image_origin(uint64_t* x, uint64_t* y, unsigned e) { sk_image_origin(x, y, e); }
void sk_host_endo_scalar(const uint64_t* k, unsigned e, uint64_t* out) {
  const bsgs_int r = sk_endo_scalar(int_of(k), e);
  memcpy(out, r.w, 32);
}
void sk_host_combine(const uint64_t* kq, const uint64_t* partial, unsigned e, uint64_t* out) {
  const bsgs_int r = sk_combine(int_of(kq), int_of(partial), e);
  memcpy(out, r.w, 32);
}
}

// k G as canonical limbs by ec.h's double-and-add; 0 for the point at infinity
static int point_of(uint64_t x[4], uint64_t y[4], const bsgs_int& k) {
  u32 kw[8], xw[8], yw[8];
  for (int i = 0; i < 4; ++i) kw[2 * i] = (u32)k.w[i], kw[2 * i + 1] = (u32)(k.w[i] >> 32);
  fe fx, fy;
  if (!ec_mul_g_affine(fx, fy, kw)) return 0;
  fe_to_words(xw, fx), fe_to_words(yw, fy);
  for (int i = 0; i < 4; ++i) x[i] = (uint64_t)xw[2 * i] | (uint64_t)xw[2 * i + 1] << 32, y[i] = (uint64_t)yw[2 * i] | (uint64_t)yw[2 * i + 1] << 32;
  return 1;
}

// self-check: for a few (k_Q, k) and every image e - the point of sk_combine(k_Q, sk_endo_scalar(k, e), e) is image e of (k_Q + k) G, and
// image e of Q = k_Q G is the point of sk_endo_scalar(k_Q, e); the edges k_Q = n - 1 and k_Q + k = 0 (mod n)
int main() {
  int bad = 0;
  const bsgs_int one = bsgs_u64(1);
  bsgs_int nm1;
  bsgs_sub(&nm1, &BSGS_N, &one);
  const bsgs_int kqs[3] = {bsgs_u64(0xdc2a04), {{0x0123456789abcdefULL, 0xfedcba9876543210ULL, 0x1f, 0}}, nm1};
  const bsgs_int ks[3] = {bsgs_u64(7), {{0x9e3779b97f4a7c15ULL, 0xbf58476d1ce4e5b9ULL, 0x94d049bb133111ebULL, 0x2545f4914f6cdd1dULL}}, bsgs_u64(1)};
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b)
      for (unsigned e = 0; e < 6; ++e) {
        const bsgs_int sum = sk_modn_add(kqs[a], ks[b]);
        const bsgs_int fin = sk_combine(kqs[a], sk_endo_scalar(ks[b], e), e);
        uint64_t x[4], y[4], wx[4], wy[4];
        const int f1 = point_of(x, y, fin), f2 = point_of(wx, wy, sum);
        bad |= f1 != f2;  // (k_Q = n - 1, k = 1: both the point at infinity, the final key 0)
        if (f1 && f2) {
          sk_image_origin(wx, wy, e);
          bad |= memcmp(x, wx, 32) != 0 || memcmp(y, wy, 32) != 0;
        }
        uint64_t qx[4], qy[4], ix[4], iy[4];
        bad |= !point_of(qx, qy, kqs[a]) || !point_of(ix, iy, sk_endo_scalar(kqs[a], e));
        sk_image_origin(qx, qy, e);
        bad |= memcmp(qx, ix, 32) != 0 || memcmp(qy, iy, 32) != 0 || !bsgs_on_curve(qx, qy);
      }
  const bsgs_int z = sk_combine(nm1, one, 0);
  bad |= (z.w[0] | z.w[1] | z.w[2] | z.w[3]) != 0;
  printf(bad ? "splitkey_host: FAILED\n" : "splitkey_host: ok\n");
  return bad;
}
