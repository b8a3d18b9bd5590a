// emit33_host.cpp — stand-alone host check of csrc/emit33.h (the addr33-only emit path of the add kernels) against the composition it
// replaces: fe_normalize + fe_to_words + fe_parity + hash160_33 + bloom_words_of / bloom_index(., 0), bit for bit.  Not part of the
// product library.  It has its own main, so this is also where a -fsanitize=undefined,address build of the device headers goes:
//   g++ -O1 -g -std=c++17 -fsanitize=undefined,address -fno-sanitize-recover=all emit33_host.cpp -o emit33_host && ./emit33_host
// usage: emit33_host                   the built-in cases (seeded random limbs at every magnitude, ceilings, multiples of p +- 1, values in
//                                      [p, 2p) after the weak pass with and without bit 24 in limb 8)
//        emit33_host cases.bin out.bin more cases from a file (tests/test_emit33_host.py writes tests/limb_cases.py's operand sets):
//                                      u32 n, then n x (x limbs[9], y limbs[9]); out.bin gets n x (h160[5], parity, index lo, index hi) of the
//                                      NEW path, which the test compares with the oracle
// Exit status 0 and a line "emit33_host: <n> cases ok" when every case agrees; the first mismatch is printed and the status is 1.
#include "../emit33.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static const u32 P_LIMBS[9] = {FE_P0, FE_P1, FE_PM, FE_PM, FE_PM, FE_PM, FE_PM, FE_PM, FE_P8};
static const u32 E = 449;  // fe256.h: the excess of a product's limb 2; the test puts it on every limb like tests/limb_cases.py

struct out_rec {
  u32 h[5], par, idx_lo, idx_hi;
};

static void old_path(out_rec& r, u32 words[9], fe x, const fe& y) {
  fe_normalize(x);
  u32 xw[8];
  fe_to_words(xw, x);
  r.par = fe_parity(y);
  hash160_33(r.h, xw, r.par);
  u64 a[5];
  bloom_words_of(a, r.h);
  const u64 idx = bloom_index(a, 0);
  r.idx_lo = (u32)idx, r.idx_hi = (u32)(idx >> 32);
  // the message words hash160_33 forms (hash160.h)
  words[0] = ((0x02u | r.par) << 24) | (xw[7] >> 8);
  for (int i = 1; i < 8; ++i) words[i] = (xw[8 - i] << 24) | (xw[7 - i] >> 8);
  words[8] = (xw[0] << 24) | 0x00800000u;
}
static void new_path(out_rec& r, u32 words[9], const fe& x, const fe& y) {
  emit33_xwords(words, x);
  r.par = emit33_parity(y);
  words[0] |= (0x02u | r.par) << 24;
  u32 o[5];
  emit33_hash(o, words);
  emit33_h160(r.h, o);
  const u64 idx = emit33_index0(o);
  r.idx_lo = (u32)idx, r.idx_hi = (u32)(idx >> 32);
}

static size_t n_cases = 0;
static bool check(const fe& x, const fe& y, out_rec* keep = nullptr) {
  out_rec a, b;
  u32 wa[9], wb[9];
  old_path(a, wa, x, y);
  new_path(b, wb, x, y);
  ++n_cases;
  bool ok = a.par == b.par && a.idx_lo == b.idx_lo && a.idx_hi == b.idx_hi;
  for (int i = 0; i < 5; ++i) ok = ok && a.h[i] == b.h[i];
  for (int i = 0; i < 9; ++i) ok = ok && wa[i] == wb[i];
  if (keep) *keep = b;
  if (ok) return true;
  printf("emit33_host: MISMATCH at case %zu\n x =", n_cases - 1);
  for (int i = 0; i < 9; ++i) printf(" %08x", x.n[i]);
  printf("\n y =");
  for (int i = 0; i < 9; ++i) printf(" %08x", y.n[i]);
  printf("\n old: parity %u index %08x%08x h160", a.par, a.idx_hi, a.idx_lo);
  for (int i = 0; i < 5; ++i) printf(" %08x", a.h[i]);
  printf("\n new: parity %u index %08x%08x h160", b.par, b.idx_hi, b.idx_lo);
  for (int i = 0; i < 5; ++i) printf(" %08x", b.h[i]);
  printf("\n old words:");
  for (int i = 0; i < 9; ++i) printf(" %08x", wa[i]);
  printf("\n new words:");
  for (int i = 0; i < 9; ++i) printf(" %08x", wb[i]);
  printf("\n");
  return false;
}

static u64 rng_state = 0x29A9E33ull;
static u64 rng() {  // splitmix64
  u64 z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static u32 below(u64 n) { return (u32)(rng() % n); }  // [0, n)

static u32 ceil_of(int i, u32 m, u32 s) { return i < 8 ? m * (1u << 29) + s : m * (1u << 24) + s; }
// limbs of magnitude m (excess s on every limb), by pattern: 0 ceilings, 1 each 0 or ceiling, 2 ceiling - 0..3, 3 uniform, 4 carry / mask edges
static fe element(u32 m, u32 s, int pat) {
  fe r;
  for (int i = 0; i < 9; ++i) {
    const u32 c = ceil_of(i, m, s);
    const u32 edge[7] = {0u, 1u, c, c - 1, c / 2, (1u << 29) - 1, 1u << 29};
    u32 v;
    switch (pat) {
    case 0: v = c; break;
    case 1: v = below(2) ? c : 0; break;
    case 2: v = c - below(4); break;
    case 3: v = below((u64)c + 1); break;
    default: v = edge[below(7)]; break;
    }
    r.n[i] = v < c ? v : c;
  }
  return r;
}
// k p + d (d small, may be negative for k >= 1) in limbs: k times p's own limbs, d on limb 0
static fe kp_plus(u32 k, int d) {
  fe r;
  for (int i = 0; i < 9; ++i) r.n[i] = k * P_LIMBS[i];
  r.n[0] += (u32)d;
  return r;
}
// a value that the weak pass leaves in [p, 2p), in a form whose limb 8 folds k: either (k + 1) p + d (limb 8 comes out of the pass at
// 2^24 - 1 with bit 24 clear), or (k + 1) 2^256 + d with the last 2^256 arriving as the carry out of limb 7 (limb 8 comes out at 2^24:
// bit 24 set); d = d_lo + d_hi 2^29
static fe weak_target(u32 k, u32 d_lo, u32 d_hi, bool bit24) {
  fe r;
  if (!bit24) {
    r = kp_plus(k + 1, 0);
  } else {
    for (int i = 0; i < 9; ++i) r.n[i] = 0;
    r.n[8] = FE_TOP + (k << 24), r.n[7] = 1u << 29;
  }
  r.n[0] += d_lo, r.n[1] += d_hi;
  return r;
}

static bool builtin_cases() {
  bool ok = true;
  // every pattern at every magnitude pair, with and without the excess
  for (u32 mx = 1; mx <= 4; ++mx)
    for (u32 my = 1; my <= 3; ++my)
      for (int px = 0; px < 5; ++px)
        for (int py = 0; py < 5; ++py)
          for (u32 s = 0; s < 2; ++s)
            for (int rep = 0; rep < (px == 0 && py == 0 ? 1 : 8); ++rep) ok = ok && check(element(mx, s * mx * E, px), element(my, s * my * E, py));
  // 20 000 seeded random inputs: uniform limbs inside random magnitudes
  for (int i = 0; i < 20000 && ok; ++i) {
    const u32 mx = 1 + below(4), my = 1 + below(3);
    ok = check(element(mx, below(2) * mx * E, 3), element(my, below(2) * my * E, 3));
  }
  // x, y = k p + d: the residues 0, 1, 2, 976, 977, p - 1, p - 2, ... in every redundant form the magnitudes allow
  const int ds[] = {0, 1, 2, 976, 977, -1, -2, -976, -977};
  for (u32 kx = 0; kx <= 4 && ok; ++kx)
    for (u32 ky = 0; ky <= 3; ++ky)
      for (int dx : ds)
        for (int dy : ds)
          if ((kx || dx >= 0) && (ky || dy >= 0)) ok = ok && check(kp_plus(kx, dx), kp_plus(ky, dy));
  // x and y in [p, 2p) after the weak pass; limb 8 with bit 24 after the pass; y == 0, 1, p - 1 beside them
  const u32 dl[] = {0, 1, 2, 976, 977, 0x1FFFFFFFu - FE_P0, 0x3D0, 0x3D1, 12345};
  for (u32 k = 0; k <= 2 && ok; ++k)
    for (u32 d0 : dl)
      for (u32 d1 = 0; d1 <= 8; ++d1)
        for (int b = 0; b < 2; ++b) {
          const fe t = weak_target(k, d0, b ? d1 : (d1 < 8 ? d1 : 7), b != 0);
          ok = ok && check(t, kp_plus(1, 0)) && check(t, kp_plus(2, 1)) && check(t, kp_plus(3, -1)) && check(kp_plus(1, 5), t) && check(t, t);
        }
  // the top of y around the value where the estimate of y >> 256 is ambiguous: limb 8 and limb 7 swept over the boundary, low limbs full / empty
  for (u32 k = 0; k <= 2 && ok; ++k)
    for (int d8 = -2; d8 <= 2; ++d8)
      for (int d7 = -3; d7 <= 3; ++d7)
        for (int low = 0; low < 3; ++low) {
          fe y;
          for (int i = 0; i < 7; ++i) y.n[i] = low == 0 ? 0u : low == 1 ? FE_M : 3u * ((1u << 29) + E);
          y.n[8] = (u32)((int)(FE_TOP + (k << 24)) + d8);
          y.n[7] = (u32)((int)FE_M + d7 * (1 << 24));
          ok = ok && check(kp_plus(0, 7), y);
          y.n[7] += 1u << 29;
          ok = ok && check(kp_plus(0, 7), y);
        }
  return ok;
}

int main(int argc, char** argv) {
  if (argc == 3) {
    FILE* f = fopen(argv[1], "rb");
    u32 n = 0;
    if (!f || fread(&n, 4, 1, f) != 1) return printf("emit33_host: cannot read %s\n", argv[1]), 2;
    std::vector<u32> in((size_t)n * 18);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return printf("emit33_host: %s is short\n", argv[1]), 2;
    fclose(f);
    std::vector<out_rec> out(n);
    for (u32 i = 0; i < n; ++i) {
      fe x, y;
      for (int l = 0; l < 9; ++l) x.n[l] = in[(size_t)i * 18 + l], y.n[l] = in[(size_t)i * 18 + 9 + l];
      if (!check(x, y, &out[i])) return 1;
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), sizeof(out_rec), n, f) != n) return printf("emit33_host: cannot write %s\n", argv[2]), 2;
    fclose(f);
  } else if (argc != 1) {
    return printf("usage: emit33_host [cases.bin out.bin]\n"), 2;
  } else if (!builtin_cases()) {
    return 1;
  }
  printf("emit33_host: %zu cases ok\n", n_cases);
  return 0;
}
