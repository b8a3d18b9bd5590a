/* bsgs_plan.h - the arithmetic of the `bsgs` command: baby-step giant-step search for the private key of a KNOWN public key Q = key G with
   a <= key <= b.  Plain C, no GPU: the CLI (cli_bsgs.h) and the host test program (csrc/tools/bsgs_host.cpp) both include this file, so
   the code that is tested is the code that runs.

   The method.  h = 2^beta baby steps, s = 2 h.
     Baby table: the x of the odd multiples (2 j - 1) G, j = 1 ... h - an ordinary walk (start scalar 1, ord_offs 1, h keys) on an
       ECL_PUB | ECL_INSERT context, which sets the filter bits of each x.
     Giant steps: W_i = (2 a + s - 1 + 2 s i) G - 2 Q, i = 0 ... N - 1, N = ceil((b - a + 1) / s) - a walk with ord_offs beta + 2 from the
       start scalar 2 a + s - 1 on an ECL_PUB | ECL_ORIGIN context with the origin O = -2 Q, probing x against the baby filter.
     Hit: x(W_i) = x((2 j - 1) G) means key = a + i s + h - 1 + (1 -+ (2 j - 1)) / 2, which lies in the window [a + i s, a + (i + 1) s - 1]:
       step i covers exactly the s keys of its window, and the windows tile [a, b] with no gap and no overlap.  A record names i, not j:
       the driver rescans window i with an ordinary ECL_PUB context and accepts a key only if all of x and the parity of y equal Q's.
     Why doubled and odd: every point the giant walk touches - lane centres, jump and table steps, group members - is (odd) G - 2 Q, which
       is the point at infinity only if 2 key is odd as an integer: impossible while 2 (b + s) + 1 < n.  So the walk never meets a zero
       x difference and a key that is itself a giant step is found like any other (with the plain form i s G - Q such a key would kill
       its whole group's shared inversion and be missed silently).  Ranges with 2 (b + s) + 1 >= n are refused. */
#ifndef BSGS_PLAN_H
#define BSGS_PLAN_H
#include <stdint.h>
#include <string.h>

typedef struct { uint64_t w[4]; } bsgs_int; /* 256-bit unsigned, little-endian limbs (the ABI's scalar layout) */

static const bsgs_int BSGS_N = {{0xbfd25e8cd0364141ULL, 0xbaaedce6af48a03bULL, 0xfffffffffffffffeULL, 0xffffffffffffffffULL}};
static const bsgs_int BSGS_P = {{0xfffffffefffffc2fULL, 0xffffffffffffffffULL, 0xffffffffffffffffULL, 0xffffffffffffffffULL}};

#define BSGS_OK 0
#define BSGS_E_ORDER 1 /* a = 0, a > b, b >= n, or beta out of 0 ... 62 */
#define BSGS_E_RANGE 2 /* 2 (b + s) + 1 >= n: a giant step could be the point at infinity */
#define BSGS_BETA_MIN 10u
#define BSGS_BETA_MAX 30u
#define BSGS_FILTER_FLOOR 1024ull   /* words of the baby filter: one per baby step, at least this many */
#define BSGS_CALL_STEPS (1ull << 32) /* giant steps per device call */

static inline int bsgs_cmp(const bsgs_int *a, const bsgs_int *b) {
  for (int i = 3; i >= 0; --i)
    if (a->w[i] != b->w[i]) return a->w[i] > b->w[i] ? 1 : -1;
  return 0;
}
static inline bsgs_int bsgs_u64(uint64_t v) { bsgs_int r = {{v, 0, 0, 0}}; return r; }
static inline uint64_t bsgs_add(bsgs_int *r, const bsgs_int *a, const bsgs_int *b) { /* returns the carry */
  unsigned __int128 c = 0;
  for (int i = 0; i < 4; ++i) c += (unsigned __int128)a->w[i] + b->w[i], r->w[i] = (uint64_t)c, c >>= 64;
  return (uint64_t)c;
}
static inline uint64_t bsgs_sub(bsgs_int *r, const bsgs_int *a, const bsgs_int *b) { /* returns the borrow */
  uint64_t br = 0;
  for (int i = 0; i < 4; ++i) {
    unsigned __int128 d = (unsigned __int128)a->w[i] - b->w[i] - br;
    r->w[i] = (uint64_t)d, br = (uint64_t)(d >> 64) & 1;
  }
  return br;
}
static inline unsigned bsgs_bits(const bsgs_int *a) { /* bit length; 0 for 0 */
  for (int i = 3; i >= 0; --i)
    if (a->w[i]) return 64u * (unsigned)i + (64u - (unsigned)__builtin_clzll(a->w[i]));
  return 0;
}
static inline bsgs_int bsgs_shl(const bsgs_int *a, unsigned n) { /* n < 256; bits shifted out are lost */
  bsgs_int r = {{0, 0, 0, 0}};
  const unsigned q = n / 64, m = n % 64;
  for (int i = 3; i >= (int)q; --i) {
    r.w[i] = a->w[i - q] << m;
    if (m && i - (int)q - 1 >= 0) r.w[i] |= a->w[i - q - 1] >> (64 - m);
  }
  return r;
}
static inline bsgs_int bsgs_shr(const bsgs_int *a, unsigned n) { /* n < 256 */
  bsgs_int r = {{0, 0, 0, 0}};
  const unsigned q = n / 64, m = n % 64;
  for (unsigned i = 0; i + q < 4; ++i) {
    r.w[i] = a->w[i + q] >> m;
    if (m && i + q + 1 < 4) r.w[i] |= a->w[i + q + 1] << (64 - m);
  }
  return r;
}

typedef struct {
  unsigned beta;
  bsgs_int a, b;
  uint64_t h, s;          /* baby steps 2^beta; keys per giant step 2^(beta + 1) */
  bsgs_int steps;         /* N = ceil((b - a + 1) / s) */
  bsgs_int baby_start;    /* the baby call: start scalar 1 ... */
  unsigned baby_offs;     /* ... ord_offs 1 ... */
  uint64_t baby_keys;     /* ... h keys */
  bsgs_int giant_start;   /* the giant walk: start scalar 2 a + s - 1 ... */
  unsigned giant_offs;    /* ... ord_offs beta + 2 (a step is 2 s) */
} bsgs_plan;

/* everything from (a, b, beta); BSGS_OK or why not */
static inline int bsgs_plan_make(bsgs_plan *p, const bsgs_int *a, const bsgs_int *b, unsigned beta) {
  const bsgs_int zero = {{0, 0, 0, 0}}, one = {{1, 0, 0, 0}};
  if (beta > 62 || bsgs_cmp(a, &zero) == 0 || bsgs_cmp(a, b) > 0 || bsgs_cmp(b, &BSGS_N) >= 0) return BSGS_E_ORDER;
  memset(p, 0, sizeof *p);
  p->beta = beta, p->a = *a, p->b = *b, p->h = 1ull << beta, p->s = 2ull << beta;
  /* the refusal: 2 (b + s) + 1 >= n  <=>  b + s >= (n - 1) / 2   (n - 1 is even; b < n < 2^256 - 2^64, so b + s does not wrap) */
  bsgs_int half, bs, s = bsgs_u64(p->s), t;
  bsgs_sub(&t, &BSGS_N, &one), half = bsgs_shr(&t, 1);
  bsgs_add(&bs, b, &s);
  if (bsgs_cmp(&bs, &half) >= 0) return BSGS_E_RANGE;
  /* N = (b - a + 1 + s - 1) >> (beta + 1) */
  bsgs_sub(&t, b, a), bsgs_add(&t, &t, &s);
  p->steps = bsgs_shr(&t, beta + 1);
  p->baby_start = one, p->baby_offs = 1, p->baby_keys = p->h;
  t = bsgs_shl(a, 1), bsgs_add(&t, &t, &s), bsgs_sub(&p->giant_start, &t, &one); /* < n by the refusal */
  p->giant_offs = beta + 2;
  return BSGS_OK;
}
/* the default beta: ceil((bits(b - a + 1) - 1) / 2), clamped to 10 ... 30 (the balance between the insert cost - 20 atomic ORs per baby key -
   and the probe cost is unmeasured: tools/bench_bsgs.py) */
static inline unsigned bsgs_default_beta(const bsgs_int *a, const bsgs_int *b) {
  const bsgs_int one = {{1, 0, 0, 0}};
  bsgs_int len;
  bsgs_sub(&len, b, a), bsgs_add(&len, &len, &one);
  const unsigned bits = bsgs_bits(&len), beta = bits / 2; /* ceil((bits - 1) / 2) */
  return beta < BSGS_BETA_MIN ? BSGS_BETA_MIN : beta > BSGS_BETA_MAX ? BSGS_BETA_MAX : beta;
}
/* words of the baby filter: one per baby step, BSGS_FILTER_FLOOR at least (20 bits set per entry in 64: a giant step passes all 20 probes
   by chance with p = (1 - e^(-20/64))^20 = 3.8e-12) */
static inline uint64_t bsgs_filter_words(const bsgs_plan *p) { return p->h > BSGS_FILTER_FLOOR ? p->h : BSGS_FILTER_FLOOR; }
/* the next call of the giant walk after `done` steps: its start scalar and how many steps it walks (at most 2^32; 0: the walk is over) */
static inline uint64_t bsgs_giant_call(const bsgs_plan *p, const bsgs_int *done, bsgs_int *start) {
  if (bsgs_cmp(done, &p->steps) >= 0) return 0;
  bsgs_int left, off = bsgs_shl(done, p->giant_offs);
  bsgs_sub(&left, &p->steps, done);
  bsgs_add(start, &p->giant_start, &off);
  return (left.w[1] | left.w[2] | left.w[3]) || left.w[0] > BSGS_CALL_STEPS ? BSGS_CALL_STEPS : left.w[0];
}
/* window i (i < N): its first key a + i s and how many keys of [a, b] it holds (s, fewer in the last one) */
static inline uint64_t bsgs_window(const bsgs_plan *p, const bsgs_int *i, bsgs_int *first) {
  bsgs_int off = bsgs_shl(i, p->beta + 1), left;
  bsgs_add(first, &p->a, &off);
  bsgs_sub(&left, &p->b, first);
  return (left.w[1] | left.w[2] | left.w[3]) || left.w[0] >= p->s ? p->s : left.w[0] + 1;
}

/* ---- the field side: y of a compressed key and the origin O = -2 Q.  Arithmetic mod p = 2^256 - 0x1000003D1 on four 64-bit limbs ---- */
#define BSGS_FP_C 0x1000003D1ull
static inline void bsgs_fp_canon(uint64_t r[4]) { /* r < 2^256 -> r mod p: r >= p iff r + C carries out */
  unsigned __int128 c = BSGS_FP_C;
  uint64_t t[4];
  for (int i = 0; i < 4; ++i) c += r[i], t[i] = (uint64_t)c, c >>= 64;
  if (c) memcpy(r, t, 32);
}
static inline void bsgs_fp_mul(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) {
  uint64_t t[8] = {0}, lo[4];
  for (int i = 0; i < 4; ++i) {
    uint64_t carry = 0;
    for (int j = 0; j < 4; ++j) {
      unsigned __int128 m = (unsigned __int128)a[i] * b[j] + t[i + j] + carry;
      t[i + j] = (uint64_t)m, carry = (uint64_t)(m >> 64);
    }
    t[i + 4] = carry;
  }
  unsigned __int128 c = 0;
  for (int i = 0; i < 4; ++i) c += (unsigned __int128)t[4 + i] * BSGS_FP_C + t[i], lo[i] = (uint64_t)c, c >>= 64;
  c *= BSGS_FP_C; /* what is left above 2^256: below 2^34 */
  for (int i = 0; i < 4; ++i) c += lo[i], lo[i] = (uint64_t)c, c >>= 64;
  if (c) { /* the sum wrapped, so it is small: once more */
    c = BSGS_FP_C;
    for (int i = 0; i < 4; ++i) c += lo[i], lo[i] = (uint64_t)c, c >>= 64;
  }
  bsgs_fp_canon(lo);
  memcpy(r, lo, 32);
}
static inline void bsgs_fp_add(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) { /* canonical in, canonical out */
  unsigned __int128 c = 0;
  uint64_t t[4];
  for (int i = 0; i < 4; ++i) c += (unsigned __int128)a[i] + b[i], t[i] = (uint64_t)c, c >>= 64;
  if (c) { /* a + b - 2^256 + C = a + b - p, below p */
    c = BSGS_FP_C;
    for (int i = 0; i < 4; ++i) c += t[i], t[i] = (uint64_t)c, c >>= 64;
  }
  bsgs_fp_canon(t);
  memcpy(r, t, 32);
}
static inline void bsgs_fp_neg(uint64_t r[4], const uint64_t a[4]) { /* p - a; 0 for 0 */
  bsgs_int x, y;
  memcpy(x.w, a, 32);
  if (!(a[0] | a[1] | a[2] | a[3])) { memset(r, 0, 32); return; }
  bsgs_sub(&y, &BSGS_P, &x);
  memcpy(r, y.w, 32);
}
static inline void bsgs_fp_sub(uint64_t r[4], const uint64_t a[4], const uint64_t b[4]) {
  uint64_t nb[4];
  bsgs_fp_neg(nb, b), bsgs_fp_add(r, a, nb);
}
static inline void bsgs_fp_pow(uint64_t r[4], const uint64_t a[4], const bsgs_int *e) {
  uint64_t acc[4] = {1, 0, 0, 0}, base[4];
  memcpy(base, a, 32);
  for (int bit = 255; bit >= 0; --bit) {
    bsgs_fp_mul(acc, acc, acc);
    if ((e->w[bit >> 6] >> (bit & 63)) & 1) bsgs_fp_mul(acc, acc, base);
  }
  memcpy(r, acc, 32);
}
static inline int bsgs_fp_below_p(const uint64_t a[4]) {
  bsgs_int x;
  memcpy(x.w, a, 32);
  return bsgs_cmp(&x, &BSGS_P) < 0;
}
/* x^3 + 7 */
static inline void bsgs_curve_rhs(uint64_t r[4], const uint64_t x[4]) {
  const uint64_t seven[4] = {7, 0, 0, 0};
  bsgs_fp_mul(r, x, x), bsgs_fp_mul(r, r, x), bsgs_fp_add(r, r, seven);
}
static inline int bsgs_on_curve(const uint64_t x[4], const uint64_t y[4]) {
  uint64_t l[4], r[4];
  if (!bsgs_fp_below_p(x) || !bsgs_fp_below_p(y)) return 0;
  bsgs_fp_mul(l, y, y), bsgs_curve_rhs(r, x);
  return !memcmp(l, r, 32);
}
/* the y of a compressed key: the square root of x^3 + 7 with the parity `odd` (p = 3 mod 4: the root is the (p + 1) / 4-th power);
   0 if x >= p or x is on no point */
static inline int bsgs_lift_x(uint64_t y[4], const uint64_t x[4], int odd) {
  const bsgs_int one = {{1, 0, 0, 0}};
  bsgs_int e;
  uint64_t r[4], t[4];
  if (!bsgs_fp_below_p(x)) return 0;
  bsgs_add(&e, &BSGS_P, &one); /* wraps past 2^256? p + 1 < 2^256: no */
  e = bsgs_shr(&e, 2);
  bsgs_curve_rhs(r, x), bsgs_fp_pow(y, r, &e);
  bsgs_fp_mul(t, y, y);
  if (memcmp(t, r, 32)) return 0;
  if ((int)(y[0] & 1) != (odd ? 1 : 0)) bsgs_fp_neg(y, y);
  return 1;
}
/* O = -2 Q for a point Q of the curve (y != 0: the curve has no point of order 2): lambda = 3 x^2 / (2 y), x' = lambda^2 - 2 x,
   y' = lambda (x - x') - y, O = (x', -y') */
static inline void bsgs_origin(uint64_t ox[4], uint64_t oy[4], const uint64_t qx[4], const uint64_t qy[4]) {
  const bsgs_int two = {{2, 0, 0, 0}};
  bsgs_int e;
  uint64_t n[4], d[4], lam[4], t[4];
  bsgs_fp_mul(t, qx, qx), bsgs_fp_add(n, t, t), bsgs_fp_add(n, n, t);
  bsgs_fp_add(d, qy, qy);
  bsgs_sub(&e, &BSGS_P, &two), bsgs_fp_pow(d, d, &e);
  bsgs_fp_mul(lam, n, d);
  bsgs_fp_mul(t, lam, lam), bsgs_fp_sub(t, t, qx), bsgs_fp_sub(ox, t, qx);
  bsgs_fp_sub(t, qx, ox), bsgs_fp_mul(t, lam, t), bsgs_fp_sub(t, t, qy);
  bsgs_fp_neg(oy, t);
}
#endif
