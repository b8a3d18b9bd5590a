// keccak.h — the Ethereum address of a secp256k1 public key, one lane = one key: the last 20 bytes of Keccak-256 over the 64 bytes
// x || y (big-endian coordinates of the uncompressed key, without the 0x04 prefix).  No reference counterpart; written from
// FIPS 202 §3 (Keccak-p[1600, 24]) with the ORIGINAL Keccak padding (first pad byte 0x01 - SHA-3 has 0x06).
//
// One absorb block: 64 message bytes, rate 136 -> pad byte 0x01 at byte 64, 0x80 at byte 135, one permutation, digest bytes 12..31.
// Written for the 32-bit VALU like hash160.h: every 64-bit lane is a pair of 32-bit words, everything is unrolled so that the round
// constants are literals and pi is register renaming;
//   theta: the five-way column parity is two v_bitop3_b32 (xor3) per half lane, and D is never formed - the lane update is the
//          three-input xor  A ^ C[x-1] ^ rotl(C[x+1], 1);
//   rho:   two v_alignbit_b32 per lane (a rotation by 32 or more swaps the halves first, which is a renaming);
//   chi:   a ^ (~b & c) is one v_bitop3_b32 (truth table 0xD2) per half lane;
//   iota:  at most two xors with literals.
// In the first round 17 of the 25 lanes are compile-time constants (15 zeros, the two padding lanes) and fold; of the last round
// only what digest bytes 12..31 need (lane 1 high half, lanes 2 and 3) is computed - iota (lane 0) not at all.
// Output convention = h160_t as in hash160.h: word k holds address bytes 4k..4k+3 big-endian.
#pragma once
#include "hash160.h"

#define KK_CHI_C(a, b, c) ((a) ^ (~(b) & (c)))
#if defined(__HIP_DEVICE_COMPILE__)
// the builtin is opaque to constant folding (hash160.h): only three run-time inputs take it, anything with a constant among its
// inputs takes the plain C form, so the first round's zero and padding lanes disappear at compile time
#define KK_ALLVAR(a, b, c) (!__builtin_constant_p(a) && !__builtin_constant_p(b) && !__builtin_constant_p(c))
H_FN u32 kk_xor3(u32 a, u32 b, u32 c) { return KK_ALLVAR(a, b, c) ? __builtin_amdgcn_bitop3_b32(a, b, c, 0x96) : XOR3_C(a, b, c); }
H_FN u32 kk_chi(u32 a, u32 b, u32 c) { return KK_ALLVAR(a, b, c) ? __builtin_amdgcn_bitop3_b32(a, b, c, 0xD2) : KK_CHI_C(a, b, c); }
#else
H_FN u32 kk_xor3(u32 a, u32 b, u32 c) { return XOR3_C(a, b, c); }
H_FN u32 kk_chi(u32 a, u32 b, u32 c) { return KK_CHI_C(a, b, c); }
#endif
H_FN u32 kk_xor5(u32 a, u32 b, u32 c, u32 d, u32 e) { return kk_xor3(kk_xor3(a, b, c), d, e); }

// rotl64 of the lane (lo, hi) by the constant r (0..63) -> two v_alignbit_b32, none for r = 0 and r = 32
H_FN void kk_rotl(u32& rlo, u32& rhi, u32 lo, u32 hi, int r) {
  if (r >= 32) {
    const u32 t = lo;
    lo = hi, hi = t, r -= 32;
  }
  if (r == 0) {
    rlo = lo, rhi = hi;
  } else {
    rlo = (lo << r) | (hi >> (32 - r));
    rhi = (hi << r) | (lo >> (32 - r));
  }
}

// rho offsets by lane index x + 5y (FIPS 202 §3.2.2, table 2) and the 24 round constants, low / high half (§3.2.5)
static constexpr int KK_RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
static constexpr u32 KK_RC_LO[24] = {0x00000001u, 0x00008082u, 0x0000808au, 0x80008000u, 0x0000808bu, 0x80000001u, 0x80008081u, 0x00008009u,
                                     0x0000008au, 0x00000088u, 0x80008009u, 0x8000000au, 0x8000808bu, 0x0000008bu, 0x00008089u, 0x00008003u,
                                     0x00008002u, 0x00000080u, 0x0000800au, 0x8000000au, 0x80008081u, 0x00008080u, 0x80000001u, 0x80008008u};
static constexpr u32 KK_RC_HI[24] = {0x00000000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x00000000u, 0x00000000u, 0x80000000u, 0x80000000u,
                                     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x80000000u,
                                     0x80000000u, 0x80000000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x80000000u, 0x00000000u, 0x80000000u};

// one round on the state a (lane x + 5y = (lo[x + 5y], hi[x + 5y]))
H_FN void keccak_round(u32 lo[25], u32 hi[25], int rnd) {
  u32 clo[5], chi[5], rlo[5], rhi[5], blo[25], bhi[25];
#pragma unroll
  for (int x = 0; x < 5; ++x) {
    clo[x] = kk_xor5(lo[x], lo[x + 5], lo[x + 10], lo[x + 15], lo[x + 20]);
    chi[x] = kk_xor5(hi[x], hi[x + 5], hi[x + 10], hi[x + 15], hi[x + 20]);
  }
#pragma unroll
  for (int x = 0; x < 5; ++x) kk_rotl(rlo[x], rhi[x], clo[x], chi[x], 1);
  // theta's update, rho and pi: B[y, 2x + 3y] = rotl(A[x, y] ^ D[x], r[x, y])
#pragma unroll
  for (int y = 0; y < 5; ++y) {
#pragma unroll
    for (int x = 0; x < 5; ++x) {
      const int i = x + 5 * y, j = y + 5 * ((2 * x + 3 * y) % 5);
      const u32 tlo = kk_xor3(lo[i], clo[(x + 4) % 5], rlo[(x + 1) % 5]);
      const u32 thi = kk_xor3(hi[i], chi[(x + 4) % 5], rhi[(x + 1) % 5]);
      kk_rotl(blo[j], bhi[j], tlo, thi, KK_RHO[i]);
    }
  }
#pragma unroll
  for (int y = 0; y < 5; ++y) {
#pragma unroll
    for (int x = 0; x < 5; ++x) {
      const int i = x + 5 * y, i1 = (x + 1) % 5 + 5 * y, i2 = (x + 2) % 5 + 5 * y;
      lo[i] = kk_chi(blo[i], blo[i1], blo[i2]);
      hi[i] = kk_chi(bhi[i], bhi[i1], bhi[i2]);
    }
  }
  lo[0] ^= KK_RC_LO[rnd];
  hi[0] ^= KK_RC_HI[rnd];
}

// xw, yw: 8 canonical little-endian u32 words each (fe_to_words of a normalised element); h: the address in h160_t words.
// The message bytes are the coordinates big-endian, the lanes little-endian: lane j = bytes 8j..8j+7, so its low half is the
// byte-swapped word 7 - 2j of the coordinate and its high half the byte-swapped word 6 - 2j.
H_FN void eth_address(u32 h[5], const u32 xw[8], const u32 yw[8]) {
  u32 lo[25], hi[25];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo[j] = bswap32(xw[7 - 2 * j]), hi[j] = bswap32(xw[6 - 2 * j]);
    lo[4 + j] = bswap32(yw[7 - 2 * j]), hi[4 + j] = bswap32(yw[6 - 2 * j]);
  }
#pragma unroll
  for (int j = 8; j < 25; ++j) lo[j] = 0, hi[j] = 0;
  lo[8] = 0x01u;         // byte 64: the first pad byte of Keccak (not SHA-3's 0x06)
  hi[16] = 0x80000000u;  // byte 135: the last byte of the rate
#pragma unroll
  for (int rnd = 0; rnd < 24; ++rnd) keccak_round(lo, hi, rnd);
  // digest bytes 12..31: lane 1 high half, lanes 2 and 3 (everything else of the last round is dead code)
  h[0] = bswap32(hi[1]);
  h[1] = bswap32(lo[2]), h[2] = bswap32(hi[2]);
  h[3] = bswap32(lo[3]), h[4] = bswap32(hi[3]);
}
