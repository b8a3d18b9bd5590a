// emit33.h — what the addr33-only add kernels (k_add<true, false, ENDO>) do with a walked point: from the raw limbs of (x, y) to the
// probe of the filter with no representation in between that the result does not need.  Same hashes, same probe, same records as
// check_point's general path (add_kernel.h: fe_normalize + fe_to_words + hash160_33 + bloom_stage1), bit for bit; the other modes keep
// that path.  What is left out:
//   * x goes from its carried limbs straight to the nine SHA-256 message words (prefix byte, x, pad): the 33-byte message is the
//     number (prefix 2^256 + x) 2^24 + 0x800000 in big-endian words, so limb i sits at bit 29 i + 24 and every word is two limbs, one
//     field extract and one shift-or.  The carry pass keeps the carried-out bits in place (the extract and the shift drop them), so no
//     limb is masked, and no 8 x 32 canonical words are formed on the way;
//   * the canonical residue differs from the weakly normalised one only when limb 8 comes out at 2^24 - 1 or above (fe_weak_ge_p needs
//     n[8] == FE_TOP or bit 24): one compare per key selects the rare exact path (2^-24 per key) instead of the full test;
//   * y is needed for one bit.  With S = sum n[i] 2^(29 i) = k 2^256 + r, r < 2^256, the canonical residue is r + k (2^32 + 977) unless
//     that reaches p, and then its parity is (n[0] ^ k) & 1.  k is read off the top: A = (n[8] << 5) + (n[7] >> 24) is floor(S / 2^227)
//     or one less (what lies below is (n[7] mod 2^24) 2^203 + n[6] 2^174 + ... < 2^227 (1 + 2^-21) for limbs below 2^32), so
//     k = A >> 29 unless the low 29 bits of A are all ones; and r + k (2^32 + 977) >= p needs r >= 2^256 - 2^37, i.e. the low 29 bits of
//     floor(S / 2^227) all ones, i.e. those of A at 2^29 - 2 or above.  That one test (2^-28 per key) selects fe_parity; otherwise no
//     carry pass at all.  n[8] << 5 needs n[8] < 2^27: y has magnitude <= 3 here;
//   * probe 0's index, a[0] << 24 | a[1] >> 24 of the h160_t words (bloom.h), is byte selections of RIPEMD-160's native chaining
//     words: one v_perm_b32 and one and-or per half, instead of four byte swaps and the 64-bit shifts.  The h160_t byte order is applied
//     where a record is parked in the ring (cand_push), not before;
//   * y of a walked point is lam b - Y (b = X - x3), and of that product the parity formula above reads bit 0 of limb 0, the top five
//     bits of limb 7 and limb 8.  emit33_ypar runs fe_mul's two streams for those alone.  Of the d stream: column 8 for its digit t8
//     (it has no carry-in, and its carry-out is not used), then columns 13..16 (k = K0 = 4 .. 7) started with no carry-in; of their
//     digits u_4 is thrown away, u_5, u_6, u_7 and the last carry dd are used.  Of the c stream: column 6 on, started at u_5 R1 - what
//     column 5 hands up less its carry x = c_5 >> 29.  No product of columns 9..12 (26) nor of columns 0..5 (21), no u_k R0 for
//     k <= 5, no u_k R1 for k <= 4, nothing of the tail past limb 8.  The operands are the walk's: a = lam of magnitude 1, b of
//     magnitude <= 6 (fe256.h: a_i <= A = 2^29 + 449, a_8 <= T = 2^24 + 449, b_i <= 6 A, b_8 <= 6 T); every column sum grows with
//     every limb, so its ceiling is its value with all limbs at theirs.
//       - The late start of the d stream.  Column 12 is five products, three of them <= 6 A^2 and two <= 6 A T, and the carry it takes
//         from column 11 (six products) is below 24.4 * 2^29: its sum is below 18.376 * 2^58 + 2^34, and what it hands to column 13 is
//         x13 < 18.4 * 2^29.  That is all the truncated column 13 lacks, so the carry it hands to column 14 is low by f,
//         0 <= f <= (x13 >> 29) + 1 <= 19, and column 14's sum D_5 is low by f and by nothing else.  Its digit u_5 = D_5 mod 2^29 comes
//         out as u_5 - f, and the carry into column 15 - with it u_6, u_7 and dd - is the true one, unless u_5 < f; and then the
//         truncated digit is u_5 - f + 2^29 >= 2^29 - 19.  One compare of the truncated digit, >= 2^29 - F with F = 32 >= 19, selects
//         the exact product (2^-24 per key); below it u_6, u_7 and dd are the true ones and u_5 is the true one less f.  No error goes
//         unguarded: u_6 and u_7 reach limb 8 through R1, and only the compare stands between a borrowed column 14 and a wrong parity.
//         (A start one column earlier, K0 = 3, lacks x12 < 24.4 * 2^29 in column 12, at most 25 in column 13 and at most 1 in column
//         14: a guard two values wide, but five more products per key.  A start one column later leaves u_5 itself without its
//         carry-in, x14 up to 12.4 * 2^29: no digit of it would be known.  K0 = 4 is the latest start that closes.)
//       - The late start of the c stream.  The low u_5 enters column 6 alone, as u_5 R1 = 256 (u_5 - f), beside the x that column
//         lacks already.  c_5 is six products <= 6 A^2 each, u_4 R1 + u_5 R0 < 2^45 and a carry below 2^35: c_5 < 36.001 * 2^58 and
//         x < 36.001 * 2^29.  Column 6 comes out low by x' = x + 256 f < 36.001 * 2^29 + 4864, its carry into column 7 low by e,
//         0 <= e <= (x' >> 29) + 1 <= 37 (64 is the bound the host program refuses to see exceeded), and so does c7, the sum of column
//         7 before it is masked.  Of c7 only bits >= 24 are read
//         (limb 7's top five bits, and the carry into limb 8 with all that follows from it: limb 8, and ct = c >> 24 of the tail), and
//         those are the true ones unless (c7 mod 2^24) + e reaches 2^24: (c7 mod 2^24) >= 2^24 - G with G = 256 >= 65 selects the exact
//         product (2^-16 per key); below it the low 24 bits of c7 are the true ones less e, no more.  G stays as it was.
//       - Bit 0 of the product's limb 0, ((a0 b0 + u_0 R0) mod 2^29 + (ct + d 2^13) 977) mod 2^29, is (a0 & b0 ^ ct) & 1: R0 and d 2^13
//         are even, 977 is odd.  y = product + 2p - Y limb-wise (fe_sub): bit 0 flips with Y's, limbs 7 and 8 get 2 p_i - Y_i.
//       - Limb 7 of y is low by e as well, so the estimate A of the item above is floor(S / 2^227) less 0, 1 or 2 here: k = A >> 29
//         unless the low 29 bits of A are at 2^29 - 2 or above, and r + k (2^32 + 977) >= p needs them at 2^29 - 3 or above.  One test,
//         (A mod 2^29) >= 2^29 - 3 (2^-27 per key), beside the guard; both select the same exact path, fe_parity(fe_mul(lam, b) - Y).
#pragma once
#include "bloom.h"
#include "hash160.h"

// D = bytes of {hi, lo} by selector (v_perm_b32: selector byte 0..3 = byte of lo, 4..7 = byte of hi)
H_FN u32 emit33_perm(u32 hi, u32 lo, u32 sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const u64 v = (u64)hi << 32 | lo;
  u32 r = 0;
  for (int i = 0; i < 4; ++i) r |= (u32)((v >> (8 * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
  return r;
#endif
}

// bits [off, off + width) of x as an opaque value: one v_bfe_u32, and the word it goes into is one v_lshl_or_b32 (left visible, the
// compiler folds the mask into a three-operand and-or and shifts both limbs of a word separately: three instructions per word)
H_FN u32 emit33_bfe(u32 x, u32 off, u32 width) {
  u32 r = (x >> off) & ((1u << width) - 1u);
  FE_HIDE24(r);
  return r;
}

// fe_normalize_weak's carry pass without the masks: c[i] & FE_M (i < 8) and c[8] are its limbs
FE_FN void emit33_carry(u32 c[9], const fe& a) {
  const u32 t = a.n[8] >> 24;
  c[0] = a.n[0] + t * 0x3D1u;
  c[1] = a.n[1] + (t << 3) + (c[0] >> 29);
#pragma unroll
  for (int i = 2; i < 8; ++i) c[i] = a.n[i] + (c[i - 1] >> 29);
  c[8] = (a.n[8] & FE_TOP) + (c[7] >> 29);
}
// SHA-256 message words 0..8 of the compressed key with x = a (any magnitude <= 7), prefix byte left zero: w[0] = x's top 24 bits
FE_FN void emit33_xwords(u32 w[9], const fe& a) {
  u32 c[9];
  emit33_carry(c, a);
  if (__builtin_expect(c[8] >= FE_TOP, 0)) {  // the only values fe_weak_ge_p can be true for
    fe t = a;
    fe_normalize(t);
#pragma unroll
    for (int i = 0; i < 9; ++i) c[i] = t.n[i];
  }
  w[0] = c[8];
  w[1] = emit33_bfe(c[6], 26, 3) | c[7] << 3;
  w[2] = emit33_bfe(c[5], 23, 6) | c[6] << 6;
  w[3] = emit33_bfe(c[4], 20, 9) | c[5] << 9;
  w[4] = emit33_bfe(c[3], 17, 12) | c[4] << 12;
  w[5] = emit33_bfe(c[2], 14, 15) | c[3] << 15;
  w[6] = emit33_bfe(c[1], 11, 18) | c[2] << 18;
  w[7] = emit33_bfe(c[0], 8, 21) | c[1] << 21;
  w[8] = c[0] << 24 | 0x00800000u;
}
// parity of the canonical residue of y, magnitude <= 3 (limb 8 below 2^27, the others below 2^32)
FE_FN u32 emit33_parity(const fe& y) {
  const u32 A = (y.n[8] << 5) + (y.n[7] >> 24);
  if (__builtin_expect((A & FE_M) >= FE_M - 1u, 0)) return fe_parity(y);
  return (y.n[0] ^ (A >> 29)) & 1u;
}
// parity of the canonical residue of a b - Y by the short way alone (a: magnitude 1, b: magnitude <= 6, Y: magnitude 1), and in `rare`
// whether it may be relied on: 0, or 1 where one of the two guards or the test on A asks for the exact product.  fe_mul's schedule with
// the d stream started at column 13 and the c stream at column 6; c7_out and u5_out (if asked for) get the low word of column 7's
// truncated sum and column 14's truncated digit, for the tests
#define EMIT33_YPAR_G 256u
#define EMIT33_YPAR_K0 4   /* the d stream starts at column 9 + K0 = 13 */
#define EMIT33_YPAR_F 32u  /* guard on column 14's truncated digit: >= 19, the most its carry-in can lack */
FE_FN u32 emit33_ypar_short(const fe& a, const fe& b, const fe& Y, u32& rare, u32* c7_out = nullptr, u32* u5_out = nullptr) {
  u64 c = 0, d = 0;
  const u32 R1 = fe_opaque(FE_R1);
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    FE_PIN64(d);
    d += (u64)a.n[i] * b.n[8 - i];
  }
  const u32 t8 = (u32)d & FE_M;  // column 8 has no carry-in: its digit is exact, its carry goes with the skipped columns
  u32 c7 = 0, u5 = 0;
#pragma unroll
  for (int k = EMIT33_YPAR_K0; k < 8; ++k) {
    if (k == EMIT33_YPAR_K0) d = (u64)a.n[k + 1] * b.n[8];  // (no carry-in)
#pragma unroll
    for (int i = k + 1 + (k == EMIT33_YPAR_K0); i < 9; ++i) {
      FE_PIN64(d);
      d += (u64)a.n[i] * b.n[9 + k - i];
    }
    const u32 u = (u32)d & FE_M;
    d >>= 29;
    if (k < 5) continue;  // u_4: shifted out, not used
    if (k == 5) u5 = u;
    if (k > 5) {
#pragma unroll
      for (int i = 0; i <= k; ++i) {
        FE_PIN64(c);
        c += (u64)a.n[i] * b.n[k - i];
      }
      FE_PIN64(c);
      c += (u64)u * FE_R0;
      if (k == 7) c7 = (u32)c;
      c >>= 29;
    }
    FE_PIN64(c);
    c += (u64)u * R1;
  }
  u32 dd = (u32)d;
  FE_HIDE24(dd);
  c += (u64)dd * FE_R0 + t8;
  const u32 ct = (u32)(c >> 24);  // (+ d << 13: even)
  const u32 y7 = (c7 & FE_M) + (2u * FE_PM - Y.n[7]);
  const u32 y8 = ((u32)c & FE_TOP) + (2u * FE_P8 - Y.n[8]);
  const u32 A = (y8 << 5) + (y7 >> 24);
  if (c7_out) *c7_out = c7;
  if (u5_out) *u5_out = u5;
  rare = (u5 >= (1u << 29) - EMIT33_YPAR_F) | ((c7 & FE_TOP) >= (1u << 24) - EMIT33_YPAR_G) | ((A & FE_M) >= FE_M - 2u);
  return ((a.n[0] & b.n[0]) ^ ct ^ Y.n[0] ^ (A >> 29)) & 1u;
}
// parity of the canonical residue of y = lam b - Y for a walked point: lam a product (magnitude 1), b = X - x3 (magnitude <= 6), Y
// magnitude 1.  path (if asked for): 1 when the exact product was taken.  This is the function as a whole, for the host program and the
// diag op (LIMB_PAR33).  The walk kernels call emit33_ypar_short themselves and go ANOTHER exact way where `rare` is set: they have
// neither lam nor b to spare by then and walk the point again (add_kernel.h: walk_ypar_step), which tests/test_gpu_par33.py reaches
// through calls of 2^18 keys and more
FE_FN u32 emit33_ypar(const fe& lam, const fe& b, const fe& Y, u32* path = nullptr) {
  u32 rare;
  u32 par = emit33_ypar_short(lam, b, Y, rare);
  if (__builtin_expect(rare != 0, 0)) par = fe_parity(fe_sub(fe_mul(lam, b), Y));
  if (path) *path = rare;
  return par;
}
// hash160 of the key whose message words 0..8 are in w (prefix byte in place): RIPEMD-160's chaining words as they come, o[i] =
// bswap32 of the h160_t word i
H_FN void emit33_hash(u32 o[5], const u32 w9[9]) {
  u32 w[16], st[8], x[16];
#pragma unroll
  for (int i = 0; i < 9; ++i) w[i] = w9[i];
#pragma unroll
  for (int i = 9; i < 15; ++i) w[i] = 0;
  w[15] = 33 * 8;
  sha256_init(st);
  sha256_compress(st, w);
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = bswap32(st[i]);
  x[8] = 0x80u;
#pragma unroll
  for (int i = 9; i < 16; ++i) x[i] = 0;
  x[14] = 256u;
  rmd160_compress_iv(o, x);
}
// bloom_index(a, 0) of bloom_words_of(h), h[i] = bswap32(o[i]):
//   high word (h0 << 24) | (h1 >> 8) | (h2 >> 24), low word (h1 << 24) | (h2 << 8) | (h3 >> 24)
H_FN u64 emit33_index0(const u32 o[5]) {
  const u32 hi = emit33_perm(o[0], o[1], 0x07000102u) | (o[2] & 0xFFu);
  const u32 lo = emit33_perm(o[2], o[3], 0x05060700u) | (o[1] & 0xFF000000u);
  return (u64)hi << 32 | lo;
}
H_FN bool emit33_probe0(const bloom_t& b, const u32 o[5]) { return bloom_bit(b, emit33_index0(o)); }
H_FN void emit33_h160(u32 h[5], const u32 o[5]) {
#pragma unroll
  for (int i = 0; i < 5; ++i) h[i] = bswap32(o[i]);
}
