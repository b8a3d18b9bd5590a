// sha512.h — SHA-512 (FIPS 180-4 §6.4) and HMAC-SHA512 (RFC 2104) for the `seed` path (bip39.h), one lane = one message.  No reference
// counterpart; host- and device-compilable like kdf.h (csrc/tools/bip39_host.cpp builds it with g++).
//
// A 64-bit word is a u64 whose halves are handled as two 32-bit words wherever that is cheaper than what the compiler makes of the
// 64-bit form (rotates, carries and three-operand adds issue in >= 4.1 clocks, xor / and / v_bitop3_b32 in 2.3-2.6):
//   rotr by n < 32 is two v_alignbit_b32 over (hi, lo) and (lo, hi); by n > 32 the same with the halves renamed; n = 32 would be a renaming;
//   Sigma / sigma are one three-way xor per half, Ch and Maj one v_bitop3_b32 per half (XOR3 / BITSEL / MAJ3 of hash160.h);
//   additions stay u64 `+`: for gfx950 the compiler emits one v_lshl_add_u64 each, no v_add_co_u32 / v_addc_co_u32 pair.
// The compression keeps the schedule as a ring of 16 words expanded in place; rounds 0..15 are one unrolled body (constant message words -
// the padding of HMAC's 64-byte messages - fold into the round constants there), rounds 16..79 a loop of four passes over a second body of
// 16, the constants of a pass read through a uniform index (scalar loads).  Two such bodies are ~2 x 16 rounds of code per compression
// instead of 80: the PBKDF2 loop, two compressions, stays far inside the 64 KB instruction cache.
#pragma once
#include "hash160.h"

H_FN u64 w64(u32 hi, u32 lo) { return ((u64)hi << 32) | lo; }
H_FN u32 hi32(u64 x) { return (u32)(x >> 32); }
H_FN u32 lo32(u64 x) { return (u32)x; }
// the low word of (hi:lo) >> n, 0 < n < 32  -> v_alignbit_b32
H_FN u32 funnel32(u32 hi, u32 lo, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, (u32)n);
#else
  return (lo >> n) | (hi << (32 - n));
#endif
}
#define S5_HI(x, n) ((n) < 32 ? funnel32(lo32(x), hi32(x), (n)) : funnel32(hi32(x), lo32(x), (n) - 32))  /* high half of rotr64(x, n), n != 32 */
#define S5_LO(x, n) ((n) < 32 ? funnel32(hi32(x), lo32(x), (n)) : funnel32(lo32(x), hi32(x), (n) - 32))
// rotr(x, a) ^ rotr(x, b) ^ rotr(x, c)
#define S5_ROT3(x, a, b, c) w64(XOR3(S5_HI(x, a), S5_HI(x, b), S5_HI(x, c)), XOR3(S5_LO(x, a), S5_LO(x, b), S5_LO(x, c)))
// rotr(x, a) ^ rotr(x, b) ^ (x >> c), c < 32
#define S5_ROT2SHR(x, a, b, c) w64(XOR3(S5_HI(x, a), S5_HI(x, b), hi32(x) >> (c)), XOR3(S5_LO(x, a), S5_LO(x, b), funnel32(hi32(x), lo32(x), (c))))
H_FN u64 sha512_S0(u64 x) { return S5_ROT3(x, 28, 34, 39); }
H_FN u64 sha512_S1(u64 x) { return S5_ROT3(x, 14, 18, 41); }
H_FN u64 sha512_s0(u64 x) { return S5_ROT2SHR(x, 1, 8, 7); }
H_FN u64 sha512_s1(u64 x) { return S5_ROT2SHR(x, 19, 61, 6); }
H_FN u64 sha512_ch(u64 e, u64 f, u64 g) { return w64(BITSEL(hi32(e), hi32(f), hi32(g)), BITSEL(lo32(e), lo32(f), lo32(g))); }
H_FN u64 sha512_maj(u64 a, u64 b, u64 c) { return w64(MAJ3(hi32(a), hi32(b), hi32(c)), MAJ3(lo32(a), lo32(b), lo32(c))); }

#if defined(__HIPCC__)
#define SHA512_K_DECL __constant__ const
#else
#define SHA512_K_DECL static const
#endif
SHA512_K_DECL u64 SHA512_K[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
    0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull,
    0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
    0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
    0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull,
    0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull,
    0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull,
    0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
// the same constants where an unrolled round wants a literal (rounds 0..15)
static constexpr u64 SHA512_K0[16] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
    0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull};

H_FN void sha512_init(u64 st[8]) {
  st[0] = 0x6a09e667f3bcc908ull, st[1] = 0xbb67ae8584caa73bull, st[2] = 0x3c6ef372fe94f82bull, st[3] = 0xa54ff53a5f1d36f1ull;
  st[4] = 0x510e527fade682d1ull, st[5] = 0x9b05688c2b3e6c1full, st[6] = 0x1f83d9abfb41bd6bull, st[7] = 0x5be0cd19137e2179ull;
}

#define SHA512_RND(a, b, c, d, e, f, g, h, kw)                  \
  {                                                             \
    const u64 t1 = h + sha512_S1(e) + sha512_ch(e, f, g) + (kw); \
    const u64 t2 = sha512_S0(a) + sha512_maj(a, b, c);          \
    d += t1;                                                    \
    h = t1 + t2;                                                \
  }
#define SHA512_EXP(w, i) (w[(i) & 15] += sha512_s1(w[((i) - 2) & 15]) + w[((i) - 7) & 15] + sha512_s0(w[((i) - 15) & 15]))

// one compression: out = in + F(in, w); w is consumed (the schedule is expanded in place).  in and out may be the same array.
H_FN void sha512_compress(u64 out[8], const u64 in[8], u64 w[16]) {
  u64 a = in[0], b = in[1], c = in[2], d = in[3], e = in[4], f = in[5], g = in[6], h = in[7];
#pragma unroll
  for (int i = 0; i < 16; i += 8) {
    SHA512_RND(a, b, c, d, e, f, g, h, SHA512_K0[i + 0] + w[i + 0]);
    SHA512_RND(h, a, b, c, d, e, f, g, SHA512_K0[i + 1] + w[i + 1]);
    SHA512_RND(g, h, a, b, c, d, e, f, SHA512_K0[i + 2] + w[i + 2]);
    SHA512_RND(f, g, h, a, b, c, d, e, SHA512_K0[i + 3] + w[i + 3]);
    SHA512_RND(e, f, g, h, a, b, c, d, SHA512_K0[i + 4] + w[i + 4]);
    SHA512_RND(d, e, f, g, h, a, b, c, SHA512_K0[i + 5] + w[i + 5]);
    SHA512_RND(c, d, e, f, g, h, a, b, SHA512_K0[i + 6] + w[i + 6]);
    SHA512_RND(b, c, d, e, f, g, h, a, SHA512_K0[i + 7] + w[i + 7]);
  }
#pragma unroll 1
  for (int r = 16; r < 80; r += 16) {
    const u64* __restrict__ k = SHA512_K + r;
#pragma unroll
    for (int i = 0; i < 16; i += 8) {
      SHA512_EXP(w, i + 0); SHA512_RND(a, b, c, d, e, f, g, h, k[i + 0] + w[i + 0]);
      SHA512_EXP(w, i + 1); SHA512_RND(h, a, b, c, d, e, f, g, k[i + 1] + w[i + 1]);
      SHA512_EXP(w, i + 2); SHA512_RND(g, h, a, b, c, d, e, f, k[i + 2] + w[i + 2]);
      SHA512_EXP(w, i + 3); SHA512_RND(f, g, h, a, b, c, d, e, k[i + 3] + w[i + 3]);
      SHA512_EXP(w, i + 4); SHA512_RND(e, f, g, h, a, b, c, d, k[i + 4] + w[i + 4]);
      SHA512_EXP(w, i + 5); SHA512_RND(d, e, f, g, h, a, b, c, k[i + 5] + w[i + 5]);
      SHA512_EXP(w, i + 6); SHA512_RND(c, d, e, f, g, h, a, b, k[i + 6] + w[i + 6]);
      SHA512_EXP(w, i + 7); SHA512_RND(b, c, d, e, f, g, h, a, k[i + 7] + w[i + 7]);
    }
  }
  out[0] = in[0] + a, out[1] = in[1] + b, out[2] = in[2] + c, out[3] = in[3] + d;
  out[4] = in[4] + e, out[5] = in[5] + f, out[6] = in[6] + g, out[7] = in[7] + h;
}

// message word j (32 bits, big-endian) of block b of the padded message whose L bytes lie at text + start: the bytes, 0x80 behind the last
// one when `pad`, zeros after it (the length words are the caller's).  The gather is kdf_gather's: two aligned words and a funnel shift,
// any start alignment, at most 7 bytes read behind the last byte (the text's two spare words).
H_FN u32 sha512_text_word(const u32* __restrict__ text, u32 start, u32 L, u32 pos, bool pad) {
  u32 v = 0;
  if (pos < L) {
    const u32 at = start + pos, sh = (at & 3u) * 8u;
    const u32 lo = text[at >> 2], hi = text[(at >> 2) + 1];
    v = bswap32((u32)((((u64)hi << 32) | lo) >> sh));
    const u32 have = L - pos;
    if (have < 4u) v &= ~(0xFFFFFFFFu >> (8u * have));
  }
  if (pad && pos <= L && L - pos < 4u) v |= 0x80000000u >> (8u * (L - pos));
  return v;
}
// SHA-512 of the L bytes at text + start
H_FN void sha512_text(u64 st[8], const u32* __restrict__ text, u32 start, u32 L) {
  sha512_init(st);
  const u32 nblk = (L + 17u + 127u) >> 7;
#pragma unroll 1
  for (u32 b = 0; b < nblk; ++b) {
    u64 w[16];
#pragma unroll
    for (u32 j = 0; j < 16; ++j)
      w[j] = w64(sha512_text_word(text, start, L, 128u * b + 8u * j, true), sha512_text_word(text, start, L, 128u * b + 8u * j + 4u, true));
    if (b == nblk - 1u) w[15] = (u64)L << 3;  // (L < 2^32: the high length word is zero, as w[14] is)
    sha512_compress(st, st, w);
  }
}

// HMAC-SHA512 with the key schedule held: ist / ost are the states after the key's ipad and opad blocks
struct hmac512 {
  u64 ist[8], ost[8];
};
// from a key block (the key, or its SHA-512 if it is longer than 128 bytes, zero-filled to 16 words)
H_FN void hmac512_key(hmac512& hm, const u64 key[16]) {
  u64 w[16], iv[8];
  sha512_init(iv);
#pragma unroll
  for (int j = 0; j < 16; ++j) w[j] = key[j] ^ 0x3636363636363636ull;
  sha512_compress(hm.ist, iv, w);
#pragma unroll
  for (int j = 0; j < 16; ++j) w[j] = key[j] ^ 0x5c5c5c5c5c5c5c5cull;
  sha512_compress(hm.ost, iv, w);
}
// the outer hash over the 64 bytes of an inner digest: eight data words, eight constant ones
H_FN void hmac512_outer(u64 out[8], const hmac512& hm, const u64 inner[8]) {
  u64 w[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = inner[j];
  w[8] = 0x8000000000000000ull;
#pragma unroll
  for (int j = 9; j < 15; ++j) w[j] = 0;
  w[15] = (128u + 64u) * 8u;
  sha512_compress(out, hm.ost, w);
}
// HMAC of a 64-byte message (PBKDF2's U_i, BIP32's master node): both compressions have that shape
H_FN void hmac512_64(u64 out[8], const hmac512& hm, const u64 msg[8]) {
  u64 w[16], inner[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = msg[j];
  w[8] = 0x8000000000000000ull;
#pragma unroll
  for (int j = 9; j < 15; ++j) w[j] = 0;
  w[15] = (128u + 64u) * 8u;
  sha512_compress(inner, hm.ist, w);
  hmac512_outer(out, hm, inner);
}
// HMAC of a message of at most 111 bytes given as its one padded block (0x80, zeros and the length 8 * (128 + bytes) in place)
H_FN void hmac512_block(u64 out[8], const hmac512& hm, const u64 block[16]) {
  u64 w[16], inner[8];
#pragma unroll
  for (int j = 0; j < 16; ++j) w[j] = block[j];
  sha512_compress(inner, hm.ist, w);
  hmac512_outer(out, hm, inner);
}
