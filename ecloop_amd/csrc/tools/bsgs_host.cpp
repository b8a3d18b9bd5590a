// bsgs_host.cpp — compiles the pieces of `bsgs` that need no GPU for the host with g++, so that the CPU test-suite can check them
// (tests/test_bsgs_host.py): the plan arithmetic the CLI runs (host/bsgs_plan.h), the origin addition of the ECL_ORIGIN set-up kernel
// (ec.h: ec_add_origin) and the bit positions the insert walk sets (pub_emit.h: pub_insert_idx).  Built as a shared object for the tests;
// it has a main of its own as well (a short self-check), so the same code can be built as a program under a sanitizer and run directly.
// Not part of the product library.
#include "../ec.h"
#include "../pub_emit.h"
#include "../../host/bsgs_plan.h"
#include <stddef.h>
#include <stdio.h>

static bsgs_int int_of(const uint64_t* w) {
  bsgs_int r;
  memcpy(r.w, w, 32);
  return r;
}

extern "C" {
// out: h, s, baby_offs, baby_keys, giant_offs, filter words, then steps[4], baby_start[4], giant_start[4]  (18 words)
int bh_plan(const uint64_t* a, const uint64_t* b, unsigned beta, uint64_t* out) {
  bsgs_plan p;
  const bsgs_int A = int_of(a), B = int_of(b);
  const int rc = bsgs_plan_make(&p, &A, &B, beta);
  if (rc != BSGS_OK) return rc;
  out[0] = p.h, out[1] = p.s, out[2] = p.baby_offs, out[3] = p.baby_keys, out[4] = p.giant_offs, out[5] = bsgs_filter_words(&p);
  memcpy(out + 6, p.steps.w, 32), memcpy(out + 10, p.baby_start.w, 32), memcpy(out + 14, p.giant_start.w, 32);
  return BSGS_OK;
}
unsigned bh_default_beta(const uint64_t* a, const uint64_t* b) {
  const bsgs_int A = int_of(a), B = int_of(b);
  return bsgs_default_beta(&A, &B);
}
// the call of the giant walk after `done` steps -> its step count (0: over, or a plan that is refused), start scalar in start[4]
uint64_t bh_giant_call(const uint64_t* a, const uint64_t* b, unsigned beta, const uint64_t* done, uint64_t* start) {
  bsgs_plan p;
  const bsgs_int A = int_of(a), B = int_of(b), D = int_of(done);
  if (bsgs_plan_make(&p, &A, &B, beta) != BSGS_OK) return 0;
  bsgs_int s;
  const uint64_t n = bsgs_giant_call(&p, &D, &s);
  if (n) memcpy(start, s.w, 32);
  return n;
}
// window i -> how many keys of [a, b] it holds, its first key in first[4]
uint64_t bh_window(const uint64_t* a, const uint64_t* b, unsigned beta, const uint64_t* i, uint64_t* first) {
  bsgs_plan p;
  const bsgs_int A = int_of(a), B = int_of(b), I = int_of(i);
  if (bsgs_plan_make(&p, &A, &B, beta) != BSGS_OK) return 0;
  bsgs_int f;
  const uint64_t n = bsgs_window(&p, &I, &f);
  memcpy(first, f.w, 32);
  return n;
}
// y of a compressed key (limbs), 0 if there is none; O = -2 Q
int bh_lift_x(const uint64_t* x, int odd, uint64_t* y) { return bsgs_lift_x(y, x, odd); }
int bh_on_curve(const uint64_t* x, const uint64_t* y) { return bsgs_on_curve(x, y); }
void bh_origin(const uint64_t* qx, const uint64_t* qy, uint64_t* ox, uint64_t* oy) { bsgs_origin(ox, oy, qx, qy); }
// the device function of k_origin_add on n items: e, o, out = canonical words x[8], y[8] per item; fin[i] = 0: the point at infinity, out
// left as the caller filled it
void bh_origin_add_many(const u32* e, const u32* o, u32* out, u32* fin, u32 n) {
  for (u32 i = 0; i < n; ++i) fin[i] = (u32)ec_add_origin(out + (size_t)i * 16, e + (size_t)i * 16, o + (size_t)i * 16);
}
// the 20 bit positions the insert walk sets for x (8 canonical words), lifted to magnitude `mag` as a walked x arrives
void bh_insert_idx_many(const u32* x, u32 mag, uint64_t* idx, u32 n) {
  for (u32 i = 0; i < n; ++i) {
    fe v = fe_from_words(x + (size_t)i * 8);
    for (u32 m = 1; m < mag; ++m) v = fe_add(v, fe_neg(fe_zero(), 0));  // + p
    u64 t[20];
    pub_insert_idx(t, v);
    for (int p = 0; p < 20; ++p) idx[(size_t)i * 20 + p] = t[p];
  }
}
}

// self-check: G + G by the origin addition against 2 G; G + (-G) reported; -2 G by bsgs_origin against it; a plan's scalars; the lift
int main() {
  const u32 gxw[8] = FE_GX_W, gyw[8] = FE_GY_W;
  u32 g[16], sum[16] = {0}, neg[16], keep[16];
  memcpy(g, gxw, 32), memcpy(g + 8, gyw, 32);
  int bad = 0;
  bad |= ec_add_origin(sum, g, g) != 1;
  uint64_t qx[4], qy[4], ox[4], oy[4], y[4];
  for (int i = 0; i < 4; ++i) qx[i] = (uint64_t)gxw[2 * i] | (uint64_t)gxw[2 * i + 1] << 32, qy[i] = (uint64_t)gyw[2 * i] | (uint64_t)gyw[2 * i + 1] << 32;
  bsgs_origin(ox, oy, qx, qy);
  bsgs_fp_neg(y, oy);  // 2 G = (ox, -oy)
  for (int i = 0; i < 4; ++i) bad |= ox[i] != ((uint64_t)sum[2 * i] | (uint64_t)sum[2 * i + 1] << 32), bad |= y[i] != ((uint64_t)sum[8 + 2 * i] | (uint64_t)sum[9 + 2 * i] << 32);
  bad |= !bsgs_on_curve(ox, oy);
  bsgs_fp_neg(y, qy);
  memcpy(neg, g, 32);
  for (int i = 0; i < 4; ++i) neg[8 + 2 * i] = (u32)y[i], neg[9 + 2 * i] = (u32)(y[i] >> 32);
  memcpy(keep, sum, sizeof keep);
  bad |= ec_add_origin(sum, g, neg) != 0 || memcmp(sum, keep, sizeof keep) != 0;
  bad |= !bsgs_lift_x(y, qx, (int)(qy[0] & 1)) || memcmp(y, qy, 32) != 0;
  bsgs_plan p;
  const bsgs_int a = bsgs_u64(0x8000), b = bsgs_u64(0x8000 + 39);
  bad |= bsgs_plan_make(&p, &a, &b, 3) != BSGS_OK || p.s != 16 || p.steps.w[0] != 3 || p.giant_start.w[0] != 2 * 0x8000 + 15 || p.giant_offs != 5;
  bsgs_int nb;
  const bsgs_int one = bsgs_u64(1);
  bsgs_sub(&nb, &BSGS_N, &one);
  bad |= bsgs_plan_make(&p, &a, &nb, 3) != BSGS_E_RANGE;
  u64 idx[20];
  pub_insert_idx(idx, fe_from_words(gxw));
  bad |= idx[0] == idx[1];
  printf(bad ? "bsgs_host: FAILED\n" : "bsgs_host: ok\n");
  return bad;
}
