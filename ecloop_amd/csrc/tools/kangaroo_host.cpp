// kangaroo_host.cpp — compiles the pieces of `kangaroo` that need no GPU for the host with g++, so that the CPU test-suite can check them
// (tests/test_kangaroo_host.py): the plan arithmetic the library and the CLI run (host/kangaroo_plan.h) and the step arithmetic of the herd
// kernel (herd_kernel.h: pick j, the zero-difference rule, the addition given the inverse, the distance add, the record packing), driven
// here lane by lane as the kernel drives it.  Built as a shared object for the tests; it has a main of its own as well (a short
// self-check), so the same code can be built as a program under a sanitizer and run directly.  Not part of the product library.
#include "../ec.h"
#include "../herd_kernel.h"
#include "../../host/kangaroo_plan.h"
#include <stddef.h>
#include <stdio.h>
#include <vector>

static bsgs_int int_of(const uint64_t* w) {
  bsgs_int r;
  memcpy(r.w, w, 32);
  return r;
}
static void words_of(u32 w[8], const uint64_t v[4]) {
  for (int i = 0; i < 4; ++i) w[2 * i] = (u32)v[i], w[2 * i + 1] = (u32)(v[i] >> 32);
}

struct kh_herd {
  u32 H = 0;
  u32 tab[HERD_TAB_WORDS];
  std::vector<fe> x, y;
  std::vector<u32> d;  // four words per kangaroo
  uint64_t zero_factors = 0;
  u32 overflow = 0;
};

extern "C" {
void kh_table(uint64_t seed, unsigned jb, uint64_t* s) {
  kg_stream st = {seed};
  kg_u128 t[KG_TABLE];
  kg_table(&st, jb, t);
  for (unsigned j = 0; j < KG_TABLE; ++j) s[2 * j] = t[j].lo, s[2 * j + 1] = t[j].hi;
}
void kh_offsets(uint64_t seed, unsigned jb, unsigned sb, uint32_t H, uint64_t* r) {
  kg_stream st = {seed};
  kg_u128 t[KG_TABLE];
  kg_table(&st, jb, t);
  for (uint32_t i = 0; i < H; ++i) {
    const kg_u128 v = kg_offset(&st, sb);
    r[2 * (size_t)i] = v.lo, r[2 * (size_t)i + 1] = v.hi;
  }
}
// a herd from the sixteen limbs of the ABI's block, as the library builds it (table and starts by ec_mul_g_affine, Q added by ec_add_origin);
// NULL if a start is the point at infinity
void* kh_new(const uint64_t* blk) {
  kh_herd* h = new kh_herd();
  const unsigned hl = (unsigned)blk[13], jb = (unsigned)blk[14], sb = (unsigned)blk[15];
  h->H = 1u << hl;
  h->x.resize(h->H), h->y.resize(h->H), h->d.resize((size_t)h->H * 4);
  kg_stream st = {blk[12]};
  kg_u128 s[KG_TABLE];
  kg_table(&st, jb, s);
  u32 in[32 * HERD_TAB_IN];
  for (u32 j = 0; j < 32; ++j) {
    const uint64_t k[4] = {s[j].lo, s[j].hi, 0, 0};
    u32 kw[8];
    words_of(kw, k);
    fe x, y;
    ec_mul_g_affine(x, y, kw);
    fe_to_words(in + j * HERD_TAB_IN, x), fe_to_words(in + j * HERD_TAB_IN + 8, y);
    for (int w = 0; w < 4; ++w) in[j * HERD_TAB_IN + 16 + w] = kw[w];
  }
  for (u32 j = 0; j < 32; ++j) herd_tab_fill(h->tab, in, j, 0), herd_tab_fill(h->tab, in, j, 1);
  u32 q[16];
  words_of(q, blk + 4), words_of(q + 8, blk + 8);
  const bsgs_int base = int_of(blk);
  for (u32 i = 0; i < h->H; ++i) {
    const kg_u128 r = kg_offset(&st, sb);
    bsgs_int k = {{r.lo, r.hi, 0, 0}};
    if (!(i & 1u) && (bsgs_add(&k, &k, &base) || bsgs_cmp(&k, &BSGS_N) >= 0)) bsgs_sub(&k, &k, &BSGS_N);
    u32 kw[8], p[16], out[16] = {0};
    words_of(kw, k.w);
    fe x, y;
    int fin = ec_mul_g_affine(x, y, kw);
    fe_to_words(p, x), fe_to_words(p + 8, y);
    if (i & 1u) {
      if (!fin) memcpy(p, q, sizeof p), fin = 1;
      else if ((fin = ec_add_origin(out, p, q)) != 0) memcpy(p, out, sizeof p);
    }
    if (!fin) {
      delete h;
      return nullptr;
    }
    h->x[i] = fe_from_words(p), h->y[i] = fe_from_words(p + 8);
    h->d[(size_t)i * 4] = (u32)r.lo, h->d[(size_t)i * 4 + 1] = (u32)(r.lo >> 32), h->d[(size_t)i * 4 + 2] = (u32)r.hi, h->d[(size_t)i * 4 + 3] = (u32)(r.hi >> 32);
  }
  return h;
}
void kh_free(void* p) { delete (kh_herd*)p; }
// `steps` jumps of every kangaroo, lane by lane as k_herd_walk makes them; records (eight words each) of the distinguished points into recs,
// up to cap; returns how many there were
uint32_t kh_run(void* p, uint32_t steps, uint32_t dp, uint32_t* recs, uint32_t cap) {
  kh_herd* h = (kh_herd*)p;
  const u32 H = h->H, L = (H + HERD_M - 1) / HERD_M, mask = dp >= 32 ? ~0u : (1u << dp) - 1u;
  uint32_t n = 0;
  fe pre[HERD_M];
  for (u32 step = 0; step < steps; ++step)
    for (u32 g = 0; g < L; ++g) {
      fe acc = fe_one();
      for (u32 m = 0; m < HERD_M; ++m) {
        const size_t i = (size_t)m * L + g;
        if (i >= H) break;
        fe tx;
        herd_jump_index(h->tab, h->x[i], tx);
        pre[m] = acc;
        const fe dx = fe_sub(tx, h->x[i]);
        if (fe_is_zero(dx)) ++h->zero_factors;
        acc = fe_mul(acc, dx);
      }
      fe inv = fe_inv(acc);
      for (u32 m = HERD_M; m-- > 0;) {
        const size_t i = (size_t)m * L + g;
        if (i >= H) continue;
        fe tx;
        const u32 j = herd_jump_index(h->tab, h->x[i], tx);
        const fe invk = fe_mul(inv, pre[m]);
        inv = fe_mul(inv, fe_sub(tx, h->x[i]));
        h->overflow |= herd_jump(h->x[i], h->y[i], &h->d[i * 4], h->tab, j, tx, invk);
        if (herd_is_dp(h->x[i], mask)) {
          if (n < cap) herd_record(recs + (size_t)n * 8, (u32)i, &h->d[i * 4], h->x[i]);
          ++n;
        }
      }
    }
  return n;
}
void kh_get(void* p, uint32_t i, uint32_t* xw, uint32_t* yw, uint32_t* d) {
  kh_herd* h = (kh_herd*)p;
  fe y = h->y[i];
  fe_normalize(y);
  fe_to_words(xw, h->x[i]), fe_to_words(yw, y);
  memcpy(d, &h->d[(size_t)i * 4], 16);
}
void kh_set(void* p, uint32_t i, const uint32_t* xw, const uint32_t* yw) {
  kh_herd* h = (kh_herd*)p;
  h->x[i] = fe_from_words(xw), h->y[i] = fe_from_words(yw);
}
// herd_is_dp on the eight canonical words of an x, with the mask k_herd_walk is given for dp bits (dp <= 32)
int kh_is_dp(const uint32_t* xw, uint32_t dp) { return herd_is_dp(fe_from_words(xw), dp >= 32 ? ~0u : (1u << dp) - 1u); }
uint64_t kh_zero_factors(void* p) { return ((kh_herd*)p)->zero_factors; }
uint32_t kh_overflow(void* p) { return ((kh_herd*)p)->overflow; }
// out: wbits, herd_log2, dp, jb, sb, round_steps, base[4]  (10 words)
int kh_plan(const uint64_t* a, const uint64_t* b, int herd_log2, int dp, uint64_t* out) {
  kg_plan p;
  const bsgs_int A = int_of(a), B = int_of(b);
  const int rc = kg_plan_make(&p, &A, &B, herd_log2, dp);
  if (rc != KG_OK) return rc;
  out[0] = p.wbits, out[1] = p.herd_log2, out[2] = p.dp, out[3] = p.jb, out[4] = p.sb, out[5] = p.round_steps;
  memcpy(out + 6, p.base.w, 32);
  return KG_OK;
}
int kh_give_up(const uint64_t* a, const uint64_t* b, int herd_log2, int dp, uint32_t max_factor, uint64_t* out) {
  kg_plan p;
  const bsgs_int A = int_of(a), B = int_of(b);
  const int rc = kg_plan_make(&p, &A, &B, herd_log2, dp);
  if (rc != KG_OK) return rc;
  const kg_u128 v = kg_give_up(&p, max_factor);
  out[0] = v.lo, out[1] = v.hi;
  return KG_OK;
}
void kh_candidates(const uint64_t* base, const uint64_t* dt, const uint64_t* dw, uint64_t* k1, uint64_t* k2) {
  const bsgs_int B = int_of(base);
  const kg_u128 t = {dt[0], dt[1]}, w = {dw[0], dw[1]};
  bsgs_int a, b;
  kg_candidates(&a, &b, &B, t, w);
  memcpy(k1, a.w, 32), memcpy(k2, b.w, 32);
}
int kh_block(const uint64_t* a, const uint64_t* b, int herd_log2, int dp, const uint64_t* qx, const uint64_t* qy, uint64_t seed, uint64_t* blk) {
  kg_plan p;
  const bsgs_int A = int_of(a), B = int_of(b);
  const int rc = kg_plan_make(&p, &A, &B, herd_log2, dp);
  if (rc == KG_OK) kg_block(blk, &p, qx, qy, seed);
  return rc;
}
}

// self-check: a herd of two for the key 0x1234 in [0x1000, 0x1fff]: after 40 jumps the tame kangaroo stands on (B + d) G and the wild one on
// (key + d) G; the records are those of the points; the candidates of a made-up pair; the refusals of the plan
int main() {
  int bad = 0;
  const bsgs_int a = bsgs_u64(0x1000), b = bsgs_u64(0x1fff);
  const uint64_t key[4] = {0x1234, 0, 0, 0};
  u32 kw[8];
  words_of(kw, key);
  fe qx, qy;
  bad |= !ec_mul_g_affine(qx, qy, kw);
  u32 qw[16];
  fe_to_words(qw, qx), fe_to_words(qw + 8, qy);
  uint64_t q[8], blk[16];
  for (int i = 0; i < 8; ++i) q[i] = (uint64_t)qw[2 * i] | (uint64_t)qw[2 * i + 1] << 32;
  bad |= kh_block(a.w, b.w, 1, 0, q, q + 4, 7, blk) != KG_OK;
  void* h = kh_new(blk);
  bad |= !h;
  if (h) {
    uint32_t recs[80 * 8];
    bad |= kh_run(h, 40, 0, recs, 80) != 80;  // dp = 0: every jump is a record
    for (u32 i = 0; i < 2; ++i) {
      u32 xw[8], yw[8], d[4], ew[8];
      kh_get(h, i, xw, yw, d);
      bsgs_int e = {{(uint64_t)d[0] | (uint64_t)d[1] << 32, (uint64_t)d[2] | (uint64_t)d[3] << 32, 0, 0}};
      const bsgs_int from = i ? bsgs_u64(0x1234) : a;
      bsgs_add(&e, &e, &from);
      words_of(ew, e.w);
      fe x, y;
      bad |= !ec_mul_g_affine(x, y, ew);
      u32 wx[8], wy[8];
      fe_to_words(wx, x), fe_to_words(wy, y);
      bad |= memcmp(wx, xw, 32) != 0 || memcmp(wy, yw, 32) != 0;
    }
    bad |= kh_zero_factors(h) != 0 || kh_overflow(h) != 0;
    kh_free(h);
  }
  bsgs_int k1, k2;
  const kg_u128 dt = {100, 0}, dw = {30, 0};
  kg_candidates(&k1, &k2, &a, dt, dw);
  bsgs_int want2;
  const bsgs_int t2 = bsgs_u64(0x1000 + 100 + 30);
  bsgs_sub(&want2, &BSGS_N, &t2);
  bad |= k1.w[0] != 0x1000 + 70 || (k1.w[1] | k1.w[2] | k1.w[3]) || bsgs_cmp(&k2, &want2) != 0;
  kg_plan p;
  const bsgs_int zero = bsgs_u64(0);
  bsgs_int wide = bsgs_shl(&a, 0);
  wide.w[1] = 1ull << 60, wide.w[0] = 0x1000;  // a + 2^124: W = 2^124 + 1
  bad |= kg_plan_make(&p, &zero, &b, -1, -1) != KG_E_ORDER || kg_plan_make(&p, &a, &BSGS_N, -1, -1) != KG_E_ORDER;
  bad |= kg_plan_make(&p, &a, &wide, -1, -1) != KG_E_WIDTH || kg_plan_make(&p, &a, &b, 25, -1) != KG_E_OPT || kg_plan_make(&p, &a, &b, -1, 33) != KG_E_OPT;
  bad |= kg_plan_make(&p, &a, &b, -1, -1) != KG_OK || p.wbits != 12 || p.sb != 12;
  printf(bad ? "kangaroo_host: FAILED\n" : "kangaroo_host: ok\n");
  return bad;
}
