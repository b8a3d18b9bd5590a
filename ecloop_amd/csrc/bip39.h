// bip39.h — the `seed` path: a BIP39 phrase to a BIP32 private key on the device (ECL_KDF_BIP39 of include/ecloop_hip.h).  No reference
// counterpart; written from BIP39 (seed = PBKDF2-HMAC-SHA512(phrase, "mnemonic" || passphrase, 2048 iterations, 64 bytes)), RFC 8018 §5.2 and
// BIP32 (master node, CKDpriv) on top of sha512.h.  Host- and device-compilable (csrc/tools/bip39_host.cpp).
//
// Two stages, one lane of the wave per phrase in both:
//   bip39_master: the phrase's bytes are gathered from the text as k_raw_scalars gathers a line (any start alignment, nothing read behind
//     the text's two spare words) into HMAC's key block - hashed first if longer than 128 bytes - and the ipad / opad states are built ONCE.
//     PBKDF2 with a 64-byte result is one block T_1: U_1 = HMAC(salt || INT(1)) - the salt, at most 111 bytes, arrives as its one padded
//     SHA-512 block, built by the host - then 2047 times U = HMAC(U), T ^= U with both states held in registers: two compressions an
//     iteration, each over eight data words and eight constant ones.  (k, c) = HMAC-SHA512("Bitcoin seed", T) is the master node: 64 bytes,
//     k as 8 little-endian words (what gtable_mul and k_mul_check* read), c as 8 big-endian words in message order.
//   bip32_ckd: one path element - I = HMAC-SHA512(c, 0x00 || ser256(k) || ser32(i)) hardened, serP(k G) || ser32(i) otherwise, the public key
//     supplied by the caller (the kernel takes it from the window table like k_verify); k <- I_L + k mod n in 32-bit limbs, c <- I_R.
// A node BIP32 calls invalid - master I_L = 0 or >= n, a child's I_L >= n, a child key 0 - is kept as k = 0, which no valid node has, and
// every descendant of it is k = 0 too: the scalar 0, which the `mul` kernels count and do not probe.
#pragma once
#include "sha512.h"

#define BIP39_ROUNDS 2048u
#define BIP39_PASS_MAX 99u   // "mnemonic" || pass || INT(1) <= 111 bytes: one SHA-512 block with its padding
#define BIP32_DEPTH_MAX 10u
#define BIP39_NODE_WORDS 16u
#ifndef BIP39_MASTER_WAVES
#define BIP39_MASTER_WAVES 4  // waves per SIMD k_bip39_master is compiled for
#endif

struct bip39_salt {  // the padded block of "mnemonic" || pass || INT(1) as the second block of HMAC's inner hash
  u64 w[16];
};
struct bip32_path {
  u32 depth, el[BIP32_DEPTH_MAX];  // bit 31 of an element: hardened
};

H_FN void bip39_salt_block(bip39_salt& s, const unsigned char* pass, u32 pass_len) {
  unsigned char b[128] = {0};
  const char* mn = "mnemonic";
  u32 len = 0;
  for (; len < 8u; ++len) b[len] = (unsigned char)mn[len];
  for (u32 i = 0; i < pass_len && i < BIP39_PASS_MAX; ++i) b[len++] = pass[i];
  b[len + 3] = 1, len += 4;  // INT(1)
  b[len] = 0x80;
  const u32 bits = (128u + len) * 8u;
  b[126] = (unsigned char)(bits >> 8), b[127] = (unsigned char)bits;
  for (int j = 0; j < 16; ++j) {
    u64 v = 0;
    for (int k = 0; k < 8; ++k) v = v << 8 | b[8 * j + k];
    s.w[j] = v;
  }
}

// secp256k1's group order as little-endian words
#define BIP32_N_WORDS {0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}
H_FN bool bip32_is_zero(const u32 a[8]) {
  u32 any = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) any |= a[i];
  return any == 0;
}
H_FN bool bip32_ge_n(const u32 a[8]) {  // a >= n: no borrow out of a - n
  const u32 n[8] = BIP32_N_WORDS;
  u32 borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u64 d = (u64)a[i] - n[i] - borrow;
    borrow = (u32)(d >> 63);
  }
  return borrow == 0;
}
// r = a + b mod n for a, b < n
H_FN void bip32_add_mod_n(u32 r[8], const u32 a[8], const u32 b[8]) {
  const u32 n[8] = BIP32_N_WORDS;
  u32 s[8], d[8], carry = 0, borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u64 t = (u64)a[i] + b[i] + carry;
    s[i] = (u32)t, carry = (u32)(t >> 32);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u64 t = (u64)s[i] - n[i] - borrow;
    d[i] = (u32)t, borrow = (u32)(t >> 63);
  }
  const bool wrap = carry || !borrow;  // the sum reached 2^256, or is >= n
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = wrap ? d[i] : s[i];
}
// a 64-byte HMAC result as a node: I_L as little-endian words, I_R in message order
H_FN void bip32_split(u32 il[8], u32 ir[8], const u64 I[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    il[2 * j] = lo32(I[3 - j]), il[2 * j + 1] = hi32(I[3 - j]);
    ir[2 * j] = hi32(I[4 + j]), ir[2 * j + 1] = lo32(I[4 + j]);
  }
}

// HMAC's key block for the L bytes at text + start
H_FN void bip39_key_block(u64 key[16], const u32* __restrict__ text, u32 start, u32 L) {
  if (L > 128u) {  // an HMAC key longer than the block is hashed first (a 24-word phrase reaches 215 bytes)
    u64 d[8];
    sha512_text(d, text, start, L);
#pragma unroll
    for (int j = 0; j < 8; ++j) key[j] = d[j], key[8 + j] = 0;
  } else {
#pragma unroll
    for (u32 j = 0; j < 16; ++j) key[j] = w64(sha512_text_word(text, start, L, 8u * j, false), sha512_text_word(text, start, L, 8u * j + 4u, false));
  }
}
// the seed of the phrase (L bytes at text + start) for the salt block `salt`: T_1 of PBKDF2-HMAC-SHA512, 2048 iterations
H_FN void bip39_seed(u64 T[8], const u32* __restrict__ text, u32 start, u32 L, const bip39_salt& salt, u32 rounds = BIP39_ROUNDS) {
  u64 key[16];
  bip39_key_block(key, text, start, L);
  hmac512 hm;
  hmac512_key(hm, key);
  u64 U[8];
  hmac512_block(U, hm, salt.w);
#pragma unroll
  for (int j = 0; j < 8; ++j) T[j] = U[j];
#pragma unroll 1
  for (u32 it = 1; it < rounds; ++it) {  // the iteration loop: ist, ost, U and T stay in registers
    hmac512_64(U, hm, U);
#pragma unroll
    for (int j = 0; j < 8; ++j) T[j] ^= U[j];
  }
}
// BIP32's validity rules on an HMAC result I = I_L || I_R.  The master node: k = I_L unless it is 0 or >= n (then 0)
H_FN void bip32_master_of(u32 node[BIP39_NODE_WORDS], const u64 I[8]) {
  u32 il[8], ir[8];
  bip32_split(il, ir, I);
  const bool valid = !bip32_is_zero(il) && !bip32_ge_n(il);
#pragma unroll
  for (int j = 0; j < 8; ++j) node[j] = valid ? il[j] : 0u, node[8 + j] = ir[j];
}
// a child: k <- I_L + k mod n, c <- I_R; false (k, c unchanged) when I_L >= n or the sum is 0
H_FN bool bip32_child_of(u32 k[8], u32 c[8], const u64 I[8]) {
  u32 il[8], ir[8], sum[8];
  bip32_split(il, ir, I);
  if (bip32_ge_n(il)) return false;
  bip32_add_mod_n(sum, il, k);
  if (bip32_is_zero(sum)) return false;
#pragma unroll
  for (int j = 0; j < 8; ++j) k[j] = sum[j], c[j] = ir[j];
  return true;
}
// the master node of a seed: (k, c) = HMAC-SHA512("Bitcoin seed", seed); k = 0 for an invalid one
H_FN void bip32_master(u32 node[BIP39_NODE_WORDS], const u64 seed[8]) {
  u64 key[16], I[8];
  key[0] = 0x426974636f696e20ull, key[1] = 0x7365656400000000ull;  // "Bitcoin seed"
#pragma unroll
  for (int j = 2; j < 16; ++j) key[j] = 0;
  hmac512 hm;
  hmac512_key(hm, key);
  hmac512_64(I, hm, seed);
  bip32_master_of(node, I);
}
// one line of the table -> its master node.  A line outside the text (the host refuses such a call before it launches) is read as empty.
H_FN void bip39_master(u32 node[BIP39_NODE_WORDS], const u32* __restrict__ text, u32 text_bytes, u64 ln, const bip39_salt& salt, u32 rounds = BIP39_ROUNDS) {
  const u32 start = (u32)ln;
  u32 L = (u32)(ln >> 32);
  if ((u64)start + L > text_bytes) L = 0;
  u64 T[8];
  bip39_seed(T, text, start, L, salt, rounds);
  bip32_master(node, T);
}

// CKDpriv: (k, c) <- child `index` of (k, c).  px / parity: x of k G (little-endian words) and the parity of its y, read only for a normal
// (not hardened) index.  -> false for an invalid child (I_L >= n or a key of 0); k and c are then left as they were.
H_FN bool bip32_ckd(u32 k[8], u32 c[8], u32 index, const u32 px[8], u32 parity) {
  u64 key[16], I[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) key[j] = w64(c[2 * j], c[2 * j + 1]);
#pragma unroll
  for (int j = 4; j < 16; ++j) key[j] = 0;
  hmac512 hm;
  hmac512_key(hm, key);
  // 37 bytes: a head byte, 32 bytes big-endian, the index, then 0x80
  const bool hard = (index >> 31) != 0;
  u32 X[8], m[10];
#pragma unroll
  for (int j = 0; j < 8; ++j) X[j] = hard ? k[7 - j] : px[7 - j];
  const u32 head = hard ? 0u : (2u | (parity & 1u));
  m[0] = head << 24 | X[0] >> 8;
#pragma unroll
  for (int j = 1; j < 8; ++j) m[j] = X[j - 1] << 24 | X[j] >> 8;
  m[8] = X[7] << 24 | index >> 8;
  m[9] = index << 24 | 0x00800000u;
  u64 blk[16];
#pragma unroll
  for (int j = 0; j < 5; ++j) blk[j] = w64(m[2 * j], m[2 * j + 1]);
#pragma unroll
  for (int j = 5; j < 15; ++j) blk[j] = 0;
  blk[15] = (128u + 37u) * 8u;
  hmac512_block(I, hm, blk);
  return bip32_child_of(k, c, I);
}

#if defined(__HIPCC__)
// the master stage: n lines of the table -> n nodes of 64 bytes.  2048 HMACs per lane and nothing else: blocks of 64, as k_raw_scalars_camp2.
__global__ void __launch_bounds__(64, BIP39_MASTER_WAVES) k_bip39_master(const u32* __restrict__ text, u32 text_bytes, const u64* __restrict__ lines, u32 n, bip39_salt salt,
                                                      u32* __restrict__ nodes) {
  const u32 i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  u32 node[BIP39_NODE_WORDS];
  bip39_master(node, text, text_bytes, lines[i], salt);
  uint4* o = (uint4*)(nodes + (size_t)i * BIP39_NODE_WORDS);
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = make_uint4(node[4 * q], node[4 * q + 1], node[4 * q + 2], node[4 * q + 3]);
}
// the path stage: node -> the scalar of the path's last element, as the 8 little-endian words k_mul_check* expects (0 for an invalid node
// anywhere on the way).  k G of a normal element by k_verify's path: the window sum over d_gtab, then one inversion.
__global__ void __launch_bounds__(64) k_bip32_path(const u32* __restrict__ nodes, u32 n, bip32_path path, const u32* __restrict__ gtab, u32* __restrict__ out) {
  const u32 i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  u32 k[8], c[8];
  const uint4* s = (const uint4*)(nodes + (size_t)i * BIP39_NODE_WORDS);
  {
    const uint4 a = s[0], b = s[1], e = s[2], f = s[3];
    k[0] = a.x, k[1] = a.y, k[2] = a.z, k[3] = a.w, k[4] = b.x, k[5] = b.y, k[6] = b.z, k[7] = b.w;
    c[0] = e.x, c[1] = e.y, c[2] = e.z, c[3] = e.w, c[4] = f.x, c[5] = f.y, c[6] = f.z, c[7] = f.w;
  }
  bool valid = !bip32_is_zero(k);
#pragma unroll 1
  for (u32 d = 0; d < path.depth; ++d) {
    u32 index = 0;
#pragma unroll
    for (u32 j = 0; j < BIP32_DEPTH_MAX; ++j) index = d == j ? path.el[j] : index;  // (a uniform select: no indexed copy of the argument)
    u32 px[8] = {0, 0, 0, 0, 0, 0, 0, 0}, parity = 0;
    if (!(index >> 31)) {
      u32 kk[9];
#pragma unroll
      for (int w = 0; w < 8; ++w) kk[w] = k[w];
      kk[8] = 0;
      fe x, y;
      jac_to_affine(x, y, gtable_mul(kk, gtab));  // (k = 0: an invalid node already, its result is dropped below)
      u32 yw[8];
      fe_to_words(px, x), fe_to_words(yw, y);
      parity = yw[0] & 1u;
    }
    valid = bip32_ckd(k, c, index, px, parity) && valid;
  }
  uint4* o = (uint4*)(out + (size_t)i * 8);
  o[0] = valid ? make_uint4(k[0], k[1], k[2], k[3]) : make_uint4(0, 0, 0, 0);
  o[1] = valid ? make_uint4(k[4], k[5], k[6], k[7]) : make_uint4(0, 0, 0, 0);
}
#endif
