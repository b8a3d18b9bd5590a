// kdf.h — the key derivation functions of `mul -raw -kdf` other than SHA-256 (which stays k_raw_scalars of mul_kernels.h): the scalar of a
// line is Keccak-256 of its bytes (`keccak`: old ethaddress, early ethercamp), SHA3-256 (`sha3`: the same sponge with the first pad
// byte 0x06) or Keccak-256 applied 2031 times (`camp2`: the later ethercamp wallet).  No reference counterpart; written from FIPS 202
// (§4 the sponge, §5.1 pad10*1, §6.1 the domain bits of SHA3) on top of keccak_round of keccak.h.
//
// The sponge: rate 136 bytes = 34 words = lanes 0..16, capacity 512 bits.  One lane of the wave per line: for every block the 34 message
// words are gathered from the text as k_raw_scalars gathers them (two aligned words and a funnel shift per word, any start alignment,
// nothing read behind the text's two spare words) and XORed into the state WITHOUT a byte swap - Keccak's lanes are little-endian, so
// message word j is the low (j even) or high (j odd) half of lane j / 2.  The padding goes in under masks: bytes of the word that holds
// the line's end are cleared behind it, the first pad byte is XORed at byte L, 0x80 at byte 135 of the last block (L = 135 mod 136:
// both in one byte, 0x81 / 0x86; L = 0 mod 136: a block of padding alone).  A line of L bytes takes L / 136 + 1 permutations; lanes of
// a wave whose lines have fewer blocks idle.  The digest is the first 32 bytes of the state: read as a big-endian 256-bit number and
// written as the 8 little-endian words k_mul_check* expects, word k of the output is the byte-swapped message-order word 7 - k.
#pragma once
#include "keccak.h"

#define KDF_RATE_WORDS 34u
#define KDF_RATE_BYTES 136u
#define KDF_PAD_KECCAK 0x01u
#define KDF_PAD_SHA3 0x06u
#define KDF_CAMP2_ROUNDS 2031u  // hashes in all: the first over the line, 2030 over the 32 bytes of the digest before

// Keccak-f[1600]: 24 rounds, unrolled (round constants are literals, pi is renaming)
H_FN void keccak_f(u32 lo[25], u32 hi[25]) {
#pragma unroll
  for (int rnd = 0; rnd < 24; ++rnd) keccak_round(lo, hi, rnd);
}

// the four bytes of the text at byte offset `at`, first byte lowest (at + 4 may lie up to 7 bytes behind the text: its spare words)
H_FN u32 kdf_gather(const u32* __restrict__ text, u32 at) {
  const u32 sh = (at & 3u) * 8u;
  const u32 lo = text[at >> 2], hi = text[(at >> 2) + 1];
  return (u32)((((u64)hi << 32) | lo) >> sh);
}

// the state after absorbing the L bytes at text + start with the first pad byte `pad`: the digest is lanes 0..3
H_FN void kdf_absorb(u32 lo[25], u32 hi[25], const u32* __restrict__ text, u32 start, u32 L, u32 pad) {
#pragma unroll
  for (int j = 0; j < 25; ++j) lo[j] = 0, hi[j] = 0;
  const u32 nblk = L / KDF_RATE_BYTES + 1u;
#pragma unroll 1
  for (u32 b = 0; b < nblk; ++b) {
#pragma unroll
    for (u32 j = 0; j < KDF_RATE_WORDS; ++j) {
      const u32 pos = KDF_RATE_BYTES * b + 4u * j;
      u32 v = 0;
      if (pos < L) {
        v = kdf_gather(text, start + pos);
        const u32 have = L - pos;
        if (have < 4u) v &= 0xFFFFFFFFu >> (32u - 8u * have);
      }
      if (pos <= L && L - pos < 4u) v ^= pad << (8u * (L - pos));
      if (j & 1u) hi[j >> 1] ^= v;
      else lo[j >> 1] ^= v;
    }
    if (b == nblk - 1u) hi[16] ^= 0x80000000u;  // byte 135 of the last block
    keccak_f(lo, hi);
  }
}

// lanes 0..3 as the scalar's 8 little-endian words (the digest read as a big-endian number)
H_FN void kdf_scalar_words(u32 w[8], const u32 lo[25], const u32 hi[25]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) w[7 - 2 * j] = bswap32(lo[j]), w[6 - 2 * j] = bswap32(hi[j]);
}

// one more Keccak-256 over the 32 bytes of the digest in lanes 0..3 (camp2's step): four data lanes, 0x01 at byte 32, 0x80 at byte 135,
// the other 19 lanes zero - the state is rebuilt from literals, so the first round folds its 21 constant lanes as eth_address folds its
// 17, and of the last round only lanes 0..3 are read: the rest of it is dead code
H_FN void kdf_rehash32(u32 lo[25], u32 hi[25]) {
  u32 a[25], c[25];
#pragma unroll
  for (int j = 0; j < 25; ++j) a[j] = j < 4 ? lo[j] : 0u, c[j] = j < 4 ? hi[j] : 0u;
  a[4] = KDF_PAD_KECCAK;
  c[16] = 0x80000000u;
  keccak_f(a, c);
#pragma unroll
  for (int j = 0; j < 4; ++j) lo[j] = a[j], hi[j] = c[j];
}

// one line of the table: the checks of k_raw_scalars (a line outside the text: bad[0], nothing read; a line behind the part of the text
// that is on the device: bad[1]), then the digest.  CAMP2: 2030 more hashes over the digest, a loop that is not unrolled around one
// unrolled permutation.
template <u32 PAD, bool CAMP2>
H_FN void kdf_line(const u32* __restrict__ text, u32 text_bytes, u32 text_have, u64 ln, u32* __restrict__ out8, u32* __restrict__ bad) {
  const u32 start = (u32)ln;
  u32 L = (u32)(ln >> 32);
  if ((u64)start + L > text_bytes) bad[0] = 1, L = 0;
  else if (start + L > text_have) bad[1] = 1, L = 0;
  u32 lo[25], hi[25];
  kdf_absorb(lo, hi, text, start, L, PAD);
  if (CAMP2) {
#pragma unroll 1
    for (u32 it = 1; it < KDF_CAMP2_ROUNDS; ++it) kdf_rehash32(lo, hi);
  }
  u32 w[8];
  kdf_scalar_words(w, lo, hi);
#pragma unroll
  for (int k = 0; k < 8; ++k) out8[k] = w[k];
}

#if defined(__HIPCC__)
// The arguments and the contract of k_raw_scalars (mul_kernels.h), one lane per line.
template <u32 PAD>
__global__ void __launch_bounds__(256) k_raw_scalars_keccak(const u32* __restrict__ text, u32 text_bytes, u32 text_have, const u64* __restrict__ lines, u32 n,
                                                             u32* __restrict__ out, u32* __restrict__ bad) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  u32 w[8];
  kdf_line<PAD, false>(text, text_bytes, text_have, lines[i], w, bad);
  uint4* o = (uint4*)(out + (size_t)i * 8);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]), o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// camp2: 2031 permutations per line - the hash is the whole cost of a key.  Blocks of 64: a piece of 2^16 lines is then 1024 workgroups,
// four per CU, instead of one block of 256 on each CU.
__global__ void __launch_bounds__(64) k_raw_scalars_camp2(const u32* __restrict__ text, u32 text_bytes, u32 text_have, const u64* __restrict__ lines, u32 n,
                                                           u32* __restrict__ out, u32* __restrict__ bad) {
  const u32 i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  u32 w[8];
  kdf_line<KDF_PAD_KECCAK, true>(text, text_bytes, text_have, lines[i], w, bad);
  uint4* o = (uint4*)(out + (size_t)i * 8);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]), o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
#endif
