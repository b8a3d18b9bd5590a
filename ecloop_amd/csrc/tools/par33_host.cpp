// par33_host.cpp — stand-alone host check of emit33_ypar (csrc/emit33.h): the parity of y = lam b - Y of a walked point from a partial
// product, against the composition it replaces, fe_parity(fe_sub(fe_mul(lam, b), Y)), and against the parity of (lam b - Y) mod p in
// big-number arithmetic of this file's own (32-bit words, schoolbook product, 2^256 = 2^32 + 977 folded until nothing is left above).
// Not part of the product library.  It has its own main, so a sanitizer build of the device headers goes here as well:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all par33_host.cpp -o par33_host && ./par33_host
// usage: par33_host [cases.bin [log2 of the random cases, default 22]]
//        par33_host -late [cases.bin [log2 of the random cases, default 22]]   (the late start of the d stream: sets 11..14 below)
// Operands at the magnitudes of the walk (add_walk.inc): lam magnitude 1, b magnitude 6, Y magnitude 1, ceilings as fe256.h defines them
// (2^29 + 449 per unit, limb 8: 2^24 + 449).  Four sets:
//   1  seeded random operand sets (a quarter of them with b's limbs at 0 or the ceiling);
//   2  limbs 5..8 of both factors at 0 or the ceiling in every one of the 256 patterns, 16 fillings of the lower limbs each;
//   3  guard cases found by a seeded search: at least 256 sets whose truncated column 7 has its low 24 bits in [2^24 - G, 2^24) (all
//      must take the exact path) and at least 256 in [2^24 - 2 G, 2^24 - G) (none may);
//   4  at least 64 sets where the truncated column 7 is wrong from bit 24 up (the dropped carry really crosses 2^24) and Y is chosen so
//      that the estimate A of y's top sits on a multiple of 2^29: the short way alone gives the WRONG parity there (checked), the
//      guarded function the right one;
//   5  four sets whose dropped carry crosses a multiple of 2^29 in column 7 with A far from any boundary: the guard alone sends them the
//      exact way (see search_cross29 for what the short way gives there).
// The search for sets 3 and 4 walks lam's limb 0 over a model of the truncated column 7 (column sums kept, three products per step; the
// d stream from column 13 on, as emit33_ypar_short runs it); every case it keeps is confirmed on emit33_ypar_short itself.
// -late checks the start of the d stream at column 13 (EMIT33_YPAR_K0 = 4) and its guard on column 14's truncated digit u5, with sets
// of its own, lines of its own ("par33_host: late: ...") and records of its own:
//   11 seeded random operand sets (another seed), the share by the exact path and by the new guard reported;
//   12 limbs 4..8 of both factors at 0 or the ceiling in every one of the 1024 patterns (the skipped columns 9..12 at their largest),
//      two fillings of the lower limbs each;
//   13 at least 256 sets whose truncated digit lies in [2^29 - F, 2^29) (all must take the exact path) and at least 256 in
//      [2^29 - 2 F, 2^29 - F) (none may);
//   14 at least 64 sets on which the late start gives a wrong u_6 (checked: column 14 borrows from column 15); the guarded function
//      is right on them.
//   On every set of 11..14: the carry the late start lacks in column 14 is f <= 19; where the guard does not fire the digit is the true
//   one less f, u_6, u_7 and the last carry are the true ones, and column 7 comes out low by e <= 64.
//   Limbs 0 and 1 do not reach columns 13 and 14, so there is no walk over them to the new guard.  Sets 13 and 14 are solved for instead:
//   one limb of the three products of column 14 is the unknown (lam_7, b_7 or b_6), the limb that would carry it into column 13 is zero
//   (b_6, lam_6 or lam_7), so column 14's sum is linear in it mod 2^29, and the other factor is odd: one modular inverse per set.
// Exit status 0 and a line "par33_host: <n> cases ok ..." with the number of cases by path; the first mismatch is printed, status 1.
// cases.bin gets u32 n, then n x (lam[9], b[9], Y[9], parity, path, set): sets 2..5 whole and the first 4096 of set 1, for the device test.
#include "../emit33.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static const u32 E = 449;
static const u32 G = EMIT33_YPAR_G;

static u64 rng_state = 0x9A833ull;
static u64 rng() {  // splitmix64
  u64 z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static u32 below(u64 n) { return (u32)(rng() % n); }  // [0, n)
static u32 ceil_of(int i, u32 m) { return i < 8 ? m * ((1u << 29) + E) : m * ((1u << 24) + E); }
// pat 0: uniform up to the ceiling, 1: each limb 0 or the ceiling, 2: ceiling - 0..3
static fe element(u32 m, int pat) {
  fe r;
  for (int i = 0; i < 9; ++i) {
    const u32 c = ceil_of(i, m);
    r.n[i] = pat == 0 ? below((u64)c + 1) : pat == 1 ? (below(2) ? c : 0u) : c - below(4);
  }
  return r;
}

// ---- big numbers: little-endian 32-bit words
struct big {
  u32 w[20];
};
static void big_add_at(big& r, int j, u64 v) {  // r += v 2^(32 j)
  for (; v && j < 20; ++j) {
    v += r.w[j];
    r.w[j] = (u32)v;
    v >>= 32;
  }
}
static big big_of(const fe& a) {
  big r;
  memset(&r, 0, sizeof r);
  for (int i = 0; i < 9; ++i) big_add_at(r, (29 * i) >> 5, (u64)a.n[i] << ((29 * i) & 31));
  return r;
}
static big big_mul(const big& a, const big& b) {  // both below 2^320
  big r;
  memset(&r, 0, sizeof r);
  for (int i = 0; i < 10; ++i) {
    u64 c = 0;
    for (int j = 0; j < 10; ++j) {
      c += (u64)a.w[i] * b.w[j] + r.w[i + j];
      r.w[i + j] = (u32)c;
      c >>= 32;
    }
    r.w[i + 10] = (u32)c;
  }
  return r;
}
// canonical residue mod p = 2^256 - 2^32 - 977 in w[0..7]
static big big_mod_p(big x) {
  for (;;) {
    bool high = false;
    for (int i = 8; i < 20; ++i) high = high || x.w[i];
    if (!high) break;
    big y;  // low 256 bits + high * (2^32 + 977)
    memset(&y, 0, sizeof y);
    for (int i = 0; i < 8; ++i) y.w[i] = x.w[i];
    for (int i = 0; i < 12; ++i) {
      big_add_at(y, i, (u64)x.w[i + 8] * 977u);
      big_add_at(y, i + 1, x.w[i + 8]);
    }
    x = y;
  }
  static const u32 P[8] = {0xFFFFFC2Fu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  bool ge = true;
  for (int i = 7; i >= 0; --i)
    if (x.w[i] != P[i]) {
      ge = x.w[i] > P[i];
      break;
    }
  if (ge) {
    u64 bw = 0;
    for (int i = 0; i < 8; ++i) {
      const u64 d = (u64)x.w[i] - P[i] - bw;
      x.w[i] = (u32)d;
      bw = (d >> 32) & 1u;
    }
  }
  return x;
}
static bool big_less(const big& a, const big& b) {  // both canonical
  for (int i = 7; i >= 0; --i)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
  return false;
}
static u32 true_parity(const fe& lam, const fe& b, const fe& Y) {
  const big m = big_mod_p(big_mul(big_of(lam), big_of(b))), y = big_mod_p(big_of(Y));
  return (m.w[0] ^ y.w[0] ^ (big_less(m, y) ? 1u : 0u)) & 1u;  // m - y, + p (odd) where that is negative
}

struct rec {
  u32 lam[9], b[9], Y[9], par, path, set;
};
static std::vector<rec> kept;
static size_t n_cases = 0, n_path[2] = {0, 0};

static void show(const char* what, const fe& lam, const fe& b, const fe& Y) {
  printf("par33_host: %s at case %zu\n lam =", what, n_cases);
  for (int i = 0; i < 9; ++i) printf(" %08x", lam.n[i]);
  printf("\n b   =");
  for (int i = 0; i < 9; ++i) printf(" %08x", b.n[i]);
  printf("\n Y   =");
  for (int i = 0; i < 9; ++i) printf(" %08x", Y.n[i]);
  printf("\n");
}
// the three parities of one operand set; path (if asked for) as emit33_ypar reports it
static bool check(const fe& lam, const fe& b, const fe& Y, u32 set, bool keep, u32* path_out = nullptr) {
  u32 path = 2;
  const u32 got = emit33_ypar(lam, b, Y, &path);
  const u32 old = fe_parity(fe_sub(fe_mul(lam, b), Y));
  const u32 want = true_parity(lam, b, Y);
  if (got != old || got != want || path > 1) {
    show("MISMATCH", lam, b, Y);
    printf(" emit33_ypar %u (path %u), fe_parity(fe_mul - Y) %u, big numbers %u\n", got, path, old, want);
    return false;
  }
  ++n_cases, ++n_path[path];
  if (path_out) *path_out = path;
  if (keep) {
    rec r;
    for (int i = 0; i < 9; ++i) r.lam[i] = lam.n[i], r.b[i] = b.n[i], r.Y[i] = Y.n[i];
    r.par = got, r.path = path, r.set = set;
    kept.push_back(r);
  }
  return true;
}

// ---- sets 3 and 4: the search.  Column sums of lam b without lam's limb 0 (the products it enters, a0 b6, a0 b7, a0 b8, are added per step)
struct colsums {
  u64 s[8], c6, c7;  // columns 9..16 (lam's limb 0 enters none of them), columns 6 and 7
};
static colsums sums_without_a0(const fe& a, const fe& b) {
  colsums r;
  memset(&r, 0, sizeof r);
  for (int k = 0; k < 8; ++k)
    for (int i = k + 1; i < 9; ++i) r.s[k] += (u64)a.n[i] * b.n[9 + k - i];
  for (int i = 1; i <= 6; ++i) r.c6 += (u64)a.n[i] * b.n[6 - i];
  for (int i = 1; i <= 7; ++i) r.c7 += (u64)a.n[i] * b.n[7 - i];
  return r;
}
static u32 model_c7(const colsums& s, u32 a0, const fe& b) {
  u64 d = 0, c = 0;
  u32 u[8];
  for (int k = EMIT33_YPAR_K0; k < 8; ++k) {  // the late start: no carry-in
    d += s.s[k];
    u[k] = (u32)d & FE_M;
    d >>= 29;
  }
  c = (u64)u[5] * FE_R1;
  c += s.c6 + (u64)a0 * b.n[6] + (u64)u[6] * FE_R0;
  c >>= 29;
  c += (u64)u[6] * FE_R1;
  c += s.c7 + (u64)a0 * b.n[7] + (u64)u[7] * FE_R0;
  return (u32)c;
}
// column 7 of the whole product as fe_mul sums it, before the mask
static u64 full_c7(const fe& a, const fe& b) {
  u64 c = 0, d = 0;
  for (int i = 0; i < 9; ++i) d += (u64)a.n[i] * b.n[8 - i];
  d >>= 29;
  for (int k = 0; k < 8; ++k) {
    for (int i = k + 1; i < 9; ++i) d += (u64)a.n[i] * b.n[9 + k - i];
    const u32 u = (u32)d & FE_M;
    d >>= 29;
    for (int i = 0; i <= k; ++i) c += (u64)a.n[i] * b.n[k - i];
    c += (u64)u * FE_R0;
    if (k == 7) return c;
    c >>= 29;
    c += (u64)u * FE_R1;
  }
  return 0;
}
// does the guard on column 14's truncated digit fire?  (lam's limb 0 has no part in it.)  Column 7's error bound holds only below it
static bool late_guard(const fe& lam, const fe& b) {
  u32 rare, u5 = 0;
  emit33_ypar_short(lam, b, fe_zero(), rare, nullptr, &u5);
  return u5 >= (1u << 29) - EMIT33_YPAR_F;
}
static fe magnitude1_y() {
  fe Y = element(1, 0);
  return Y;
}
static bool search_sets() {
  size_t inside = 0, under = 0, wrong = 0, largest_e = 0;
  for (u64 round = 0; inside < 256 || under < 256 || wrong < 64; ++round) {
    if (round >= (1u << 18)) return printf("par33_host: the search found %zu inside, %zu below, %zu wrong cases only\n", inside, under, wrong), false;
    fe lam = element(1, 0);
    const fe b = element(6, round & 1 ? 2 : 0);  // every other round: b at its ceiling, the largest dropped carries
    if (late_guard(lam, b)) continue;  // (2^-24)
    const colsums s = sums_without_a0(lam, b);
    const u32 a0 = below((1u << 29) - 1024);
    for (u32 step = 0; step < 1024; ++step) {
      const u32 lo = model_c7(s, a0 + step, b) & FE_TOP;
      if (lo < (1u << 24) - 2 * G) continue;
      lam.n[0] = a0 + step;
      const bool in = lo >= (1u << 24) - G;
      fe Y = magnitude1_y();
      u32 rare, c7 = 0;
      u32 par_short = emit33_ypar_short(lam, b, Y, rare, &c7);
      if ((c7 & FE_TOP) != lo) return show("the model of the search disagrees with emit33_ypar_short", lam, b, Y), false;
      if (!in && rare) continue;  // (the test on A fired beside the guard: 2^-27)
      if (in ? inside < 512 : under < 512) {
        u32 path;
        if (!check(lam, b, Y, 3, true, &path)) return false;
        if (path != (in ? 1u : 0u)) return show(in ? "inside the guard, but not the exact path" : "below the guard, but the exact path", lam, b, Y), false;
        in ? ++inside : ++under;
      }
      if (!in || wrong >= 128) continue;
      // set 4: the dropped carry crosses 2^24 (and not 2^29: limb 8 and ct stay as they are)
      const u64 t = full_c7(lam, b);
      const u32 e = (u32)t - c7;
      if (e > 64) return show("the carry error is outside [0, 64]", lam, b, Y), false;
      if (e > largest_e) largest_e = e;
      if (((u32)t >> 24) == (c7 >> 24) || (t >> 29) != ((t - e) >> 29)) continue;
      const fe m = fe_mul(lam, b);
      if (m.n[7] != ((u32)t & FE_M)) return show("limb 7 of fe_mul is not column 7", lam, b, Y), false;
      // Y: limb 7 with 2 p_7 - Y_7 = j 2^24 (j = 32..63) so that h = (y_7 >> 24) is a multiple of 32, limb 8 so that A = 32 y_8 + h
      // is a multiple of 2^29
      u32 j = 32;
      while (((m.n[7] >> 24) + j) & 31u) ++j;
      const u32 h = (m.n[7] >> 24) + j;
      Y.n[7] = 2u * FE_PM - (j << 24);
      Y.n[8] = (m.n[8] + 2u * FE_P8 + (h >> 5)) & FE_TOP;
      par_short = emit33_ypar_short(lam, b, Y, rare, &c7);
      if (par_short == true_parity(lam, b, Y) || !rare) return show("the short way alone is NOT wrong where it should be", lam, b, Y), false;
      u32 path;
      if (!check(lam, b, Y, 4, true, &path)) return false;
      if (path != 1) return show("set 4, but not the exact path", lam, b, Y), false;
      ++wrong;
    }
  }
  printf("par33_host: search: %zu inside the guard, %zu just below, %zu where the short way alone is wrong; largest carry error %zu\n", inside, under, wrong, largest_e);
  return true;
}

// ---- set 5: the dropped carry crosses a multiple of 2^29 in column 7, so that the truncated stream hands limb 8 one too little (and limb 7
// comes out near 2^29 instead of near 0).  Only the guard stands there: Y is taken so that A is nowhere near a multiple of 2^29 and the test
// on A cannot fire.  As a VALUE the truncated limbs are still the true ones less e 2^203, so the short parity is wrong on such a set only
// if limb 8 wraps as well (its 24 bits all ones before the carry: 2^-24 on top of 2^-24) - the program counts those it meets and prints
// the count; what it asserts is that each set goes the exact way and comes out right
static bool search_cross29() {
  size_t found = 0, short_wrong = 0;
  for (u64 round = 0; found < 4; ++round) {
    if (round >= (1u << 16)) return printf("par33_host: the search found %zu sets that cross 2^29 only\n", found), false;
    fe lam = element(1, 0);
    const fe b = element(6, 2);
    if (late_guard(lam, b)) continue;
    const colsums s = sums_without_a0(lam, b);
    const u32 a0 = below((1u << 29) - (1u << 16));
    for (u32 step = 0; step < (1u << 16) && found < 4; ++step) {
      if ((model_c7(s, a0 + step, b) & FE_M) < FE_M - 64u) continue;
      lam.n[0] = a0 + step;
      fe Y = element(1, 0);
      u32 rare, c7 = 0;
      u32 par_short = emit33_ypar_short(lam, b, Y, rare, &c7);
      const u64 t = full_c7(lam, b);
      const u32 e = (u32)t - c7;
      if (e > 64) return show("the carry error is outside [0, 64]", lam, b, Y), false;
      if ((t >> 29) == ((t - e) >> 29)) continue;  // (near, but not across)
      for (int tries = 0; tries < 64; ++tries) {  // A well inside its range of 2^29
        const fe y = fe_sub(fe_mul(lam, b), Y);
        const u32 A = ((y.n[8] << 5) + (y.n[7] >> 24)) & FE_M;
        if (A >= 64u && A <= FE_M - 64u) break;
        Y = element(1, 0);
      }
      par_short = emit33_ypar_short(lam, b, Y, rare, &c7);
      if (!rare || (c7 & FE_TOP) < (1u << 24) - G) return show("across 2^29, but the guard did not fire", lam, b, Y), false;
      if (par_short != true_parity(lam, b, Y)) ++short_wrong;
      u32 path;
      if (!check(lam, b, Y, 5, true, &path)) return false;
      if (path != 1) return show("set 5, but not the exact path", lam, b, Y), false;
      ++found;
    }
  }
  printf("par33_host: %zu sets whose dropped carry crosses 2^29 in column 7 (the guard alone sends them the exact way), %zu of them wrong by the short way\n", found, short_wrong);
  return true;
}

// ---- -late: the d stream from column 13 on and the guard on column 14's truncated digit (sets 11..14)
static const u32 F = EMIT33_YPAR_F, F_MOST = 19;  // the guard's width; the most the carry into column 14 may lack (emit33.h)
struct dstream {
  u32 u[8];      // the digits of columns 9..16
  u64 carry[8];  // what each hands up
};
// fe_mul's d stream from column 9 + k0 on with no carry-in (k0 < 0: the whole stream, with column 8's carry)
static dstream d_digits(const fe& a, const fe& b, int k0) {
  dstream r;
  memset(&r, 0, sizeof r);
  u64 d = 0;
  if (k0 < 0) {
    for (int i = 0; i < 9; ++i) d += (u64)a.n[i] * b.n[8 - i];
    d >>= 29;
  }
  for (int k = k0 < 0 ? 0 : k0; k < 8; ++k) {
    for (int i = k + 1; i < 9; ++i) d += (u64)a.n[i] * b.n[9 + k - i];
    r.u[k] = (u32)d & FE_M;
    d >>= 29;
    r.carry[k] = d;
  }
  return r;
}
static size_t late_guarded = 0, late_largest_f = 0, late_largest_e = 0, late_borrows = 0;
// one operand set of the late mode: what emit33.h derives for the late start, then the three parities.  borrowed (if asked for): whether
// the late start alone gives a wrong u_6
static bool late_check(const fe& lam, const fe& b, const fe& Y, u32 set, bool keep, u32* path_out = nullptr, bool* borrowed = nullptr) {
  const dstream t = d_digits(lam, b, -1), s = d_digits(lam, b, EMIT33_YPAR_K0);
  const u64 f = t.carry[4] - s.carry[4];
  if (f > F_MOST) return show("column 14 lacks more than 19", lam, b, Y), false;
  if (f > late_largest_f) late_largest_f = f;
  u32 rare, c7 = 0, u5 = 0;
  emit33_ypar_short(lam, b, Y, rare, &c7, &u5);
  if (u5 != s.u[5]) return show("the model of the late start disagrees with emit33_ypar_short", lam, b, Y), false;
  const bool fires = u5 >= (1u << 29) - F, wrong6 = s.u[6] != t.u[6];
  if (fires && !rare) return show("inside the guard on column 14, but not flagged", lam, b, Y), false;
  if (wrong6 && (!fires || t.u[5] >= f || s.u[5] != t.u[5] + (1u << 29) - (u32)f || s.carry[5] + 1 != t.carry[5]))
    return show("a wrong u_6 that is no borrow of column 14 under the guard", lam, b, Y), false;
  if (!wrong6) {
    if (s.u[5] + (u32)f != t.u[5] || s.u[7] != t.u[7] || s.carry[7] != t.carry[7]) return show("the late start is wrong past u_5 - f", lam, b, Y), false;
    const u32 e = (u32)full_c7(lam, b) - c7;
    if (e > 64) return show("the carry error of column 7 is outside [0, 64]", lam, b, Y), false;
    if (e > late_largest_e) late_largest_e = e;
  }
  late_guarded += fires, late_borrows += wrong6;
  if (borrowed) *borrowed = wrong6;
  return check(lam, b, Y, set, keep, path_out);
}
static u32 inverse29(u32 x) {  // of an odd x mod 2^29
  u32 r = x;
  for (int i = 0; i < 5; ++i) r *= 2u - x * r;
  return r & FE_M;
}
// sets 13 and 14: operand sets whose truncated digit of column 14 is `target`
static bool late_solve(fe& lam, fe& b, u32 target, int knob) {
  u32 *zero = knob == 0 ? &b.n[6] : knob == 1 ? &lam.n[6] : &lam.n[7], *x = knob == 0 ? &lam.n[7] : knob == 1 ? &b.n[7] : &b.n[6];
  u32* by = knob == 0 ? &b.n[7] : knob == 1 ? &lam.n[7] : &lam.n[8];
  *zero = 0, *x = 0;
  if (!(*by & 1u)) *by = *by ? *by - 1 : 1u;  // odd, and still under its ceiling
  const u32 now = d_digits(lam, b, EMIT33_YPAR_K0).u[5];
  *x = (u32)(((u64)((target - now) & FE_M) * inverse29(*by)) & FE_M);
  if (knob) *x += below(6) << 29;  // b's limbs: magnitude 6
  return d_digits(lam, b, EMIT33_YPAR_K0).u[5] == target;
}
static bool late_sets() {
  size_t inside = 0, under = 0, wrong = 0;
  for (u64 round = 0; inside < 256 || under < 256 || wrong < 64; ++round) {
    if (round >= (1u << 16)) return printf("par33_host: late: the search found %zu inside, %zu below, %zu wrong cases only\n", inside, under, wrong), false;
    fe lam = element(1, 0), b = element(6, round & 1 ? 2 : 0);  // every other round: b at its ceiling, the largest missing carries
    const int want = (int)(round % 3);                          // 0: inside, 1: just below, 2: the top two values of the digit (a borrow where f > 1)
    const u32 target = want == 2 ? FE_M - below(2) : (1u << 29) - (want ? 2 * F : F) + below(F);
    if (!late_solve(lam, b, target, (int)((round / 3) % 3))) return show("late_solve missed its target", lam, b, fe_zero()), false;
    const fe Y = element(1, 0);
    u32 rare, u5 = 0, path;
    emit33_ypar_short(lam, b, Y, rare, nullptr, &u5);
    if (u5 != target) return show("the model of the late start disagrees with emit33_ypar_short", lam, b, Y), false;
    if (want == 1 && rare) continue;  // (another test fired beside the guard: 2^-16)
    bool borrowed;
    if (want == 2) {
      if (wrong >= 128) continue;
      if (d_digits(lam, b, -1).u[6] == d_digits(lam, b, EMIT33_YPAR_K0).u[6]) continue;  // (f was 0 or 1: no borrow)
      if (!late_check(lam, b, Y, 14, true, &path, &borrowed)) return false;
      if (!borrowed || path != 1) return show("set 14, but no wrong u_6 or not the exact path", lam, b, Y), false;
      ++wrong;
      continue;
    }
    if (!late_check(lam, b, Y, 13, true, &path, &borrowed)) return false;
    if (path != (want ? 0u : 1u)) return show(want ? "below the guard on column 14, but the exact path" : "inside the guard on column 14, but not the exact path", lam, b, Y), false;
    want ? ++under : ++inside;
  }
  printf("par33_host: late: search: %zu inside the guard, %zu just below, %zu where the late start alone gives a wrong u_6\n", inside, under, wrong);
  return true;
}
static int late_main(const char* out, int lg) {
  rng_state = 0x1A7E57A87ull;
  // set 11
  const size_t n1 = (size_t)1 << lg;
  for (size_t i = 0; i < n1; ++i)
    if (!late_check(element(1, 0), element(6, (i & 3) == 3 ? 1 : 0), element(1, 0), 11, i < 1024)) return 1;
  printf("par33_host: late: set 11: %zu random cases, %zu by the exact path, %zu of them inside the guard on column 14\n", n1, n_path[1], late_guarded);
  if (n_path[1] * 4096 > n1) return printf("par33_host: late: more than one case in 2^12 by the exact path\n"), 1;
  // set 12
  for (u32 pat = 0; pat < 1024; ++pat)
    for (int rep = 0; rep < 2; ++rep) {
      fe lam = element(1, rep ? 2 : 0), b = element(6, rep ? 2 : 0);
      for (int i = 0; i < 5; ++i) {
        lam.n[4 + i] = (pat >> i) & 1u ? ceil_of(4 + i, 1) : 0u;
        b.n[4 + i] = (pat >> (5 + i)) & 1u ? ceil_of(4 + i, 6) : 0u;
      }
      if (!late_check(lam, b, element(1, rep ? 0 : 2), 12, true)) return 1;
    }
  printf("par33_host: late: set 12: 1024 patterns of limbs 4..8; column 14 lacks at most %zu so far, column 7 at most %zu\n", late_largest_f, late_largest_e);
  if (late_largest_f + 1 < F_MOST) return printf("par33_host: late: the patterns do not reach the ceiling in column 14 (18 or 19)\n"), 1;
  // sets 13 and 14
  if (!late_sets()) return 1;
  if (out) {
    FILE* f = fopen(out, "wb");
    const u32 n = (u32)kept.size();
    if (!f || fwrite(&n, 4, 1, f) != 1 || fwrite(kept.data(), sizeof(rec), n, f) != n) return printf("par33_host: cannot write %s\n", out), 2;
    fclose(f);
  }
  printf("par33_host: late: largest carry lacking in column 14 %zu, in column 7 %zu; %zu sets with a wrong u_6 by the late start alone\n", late_largest_f, late_largest_e, late_borrows);
  printf("par33_host: late: %zu cases ok, %zu by the short way, %zu by the exact path\n", n_cases, n_path[0], n_path[1]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "-late")) {
    const int lg = argc == 4 ? atoi(argv[3]) : 22;
    if (argc > 4 || lg < 12 || lg > 30) return printf("usage: par33_host -late [cases.bin [log2 of the random cases, 12 .. 30]]\n"), 2;
    return late_main(argc >= 3 ? argv[2] : nullptr, lg);
  }
  if (argc > 3) return printf("usage: par33_host [cases.bin [log2 of the random cases]]\n"), 2;
  const int lg = argc == 3 ? atoi(argv[2]) : 22;
  if (lg < 12 || lg > 30) return printf("par33_host: log2 of the random cases: 12 .. 30\n"), 2;
  // set 1
  const size_t n1 = (size_t)1 << lg;
  for (size_t i = 0; i < n1; ++i)
    if (!check(element(1, 0), element(6, (i & 3) == 3 ? 1 : 0), element(1, 0), 1, i < 4096)) return 1;
  const size_t exact1 = n_path[1];
  printf("par33_host: set 1: %zu random cases, %zu by the exact path\n", n1, exact1);
  if (exact1 * 4096 > n1) return printf("par33_host: more than one case in 2^12 by the exact path\n"), 1;
  // set 2
  for (u32 pat = 0; pat < 256; ++pat)
    for (int rep = 0; rep < 16; ++rep) {
      fe lam = element(1, rep % 3), b = element(6, (rep / 3) % 3);
      for (int i = 0; i < 4; ++i) {
        lam.n[5 + i] = (pat >> i) & 1u ? ceil_of(5 + i, 1) : 0u;
        b.n[5 + i] = (pat >> (4 + i)) & 1u ? ceil_of(5 + i, 6) : 0u;
      }
      if (!check(lam, b, element(1, rep & 1 ? 0 : 2), 2, true)) return 1;
    }
  // sets 3 and 4
  if (!search_sets()) return 1;
  if (!search_cross29()) return 1;
  if (argc >= 2) {
    FILE* f = fopen(argv[1], "wb");
    const u32 n = (u32)kept.size();
    if (!f || fwrite(&n, 4, 1, f) != 1 || fwrite(kept.data(), sizeof(rec), n, f) != n) return printf("par33_host: cannot write %s\n", argv[1]), 2;
    fclose(f);
  }
  printf("par33_host: %zu cases ok, %zu by the short way, %zu by the exact path\n", n_cases, n_path[0], n_path[1]);
  return 0;
}
