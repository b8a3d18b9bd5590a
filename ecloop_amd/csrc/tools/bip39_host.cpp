// bip39_host.cpp — compiles the DEVICE headers sha512.h / bip39.h (the bodies of k_bip39_master and k_bip32_path without the public key of
// a normal element, which the kernel takes from the window table and a caller supplies here) for the host with g++, so that the CPU
// test-suite can check SHA-512, HMAC, PBKDF2, the gather, CKDpriv and the node validity rules without a GPU (tests/test_seed_host.py).
// Built as a shared object for the tests; it has a main of its own as well - known answers, and every length at every alignment in a heap
// buffer that ends with the text's two spare words - so the same code can be built as a program under a sanitizer and run directly.  Not
// part of the product library.
#include "../bip39.h"
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" {
// SHA-512 of every line: out[8 i ..] = the digest's eight 64-bit words
void bh_sha512(const u32* text, const u64* lines, u32 n, u64* out) {
  for (u32 i = 0; i < n; ++i) sha512_text(out + (size_t)i * 8, text, (u32)lines[i], (u32)(lines[i] >> 32));
}
// HMAC-SHA512 with the line `key` as the key over msg (at most 111 bytes; 64 bytes go through hmac512_64 as well and must agree)
int bh_hmac(const u32* text, u64 key, const unsigned char* msg, u32 msg_len, u64* out) {
  if (msg_len > 111u) return -1;
  u64 kb[16], blk[16];
  bip39_key_block(kb, text, (u32)key, (u32)(key >> 32));
  hmac512 hm;
  hmac512_key(hm, kb);
  unsigned char b[128] = {0};
  memcpy(b, msg, msg_len);
  b[msg_len] = 0x80;
  const u32 bits = (128u + msg_len) * 8u;
  b[126] = (unsigned char)(bits >> 8), b[127] = (unsigned char)bits;
  for (int j = 0; j < 16; ++j) {
    u64 v = 0;
    for (int k = 0; k < 8; ++k) v = v << 8 | b[8 * j + k];
    blk[j] = v;
  }
  hmac512_block(out, hm, blk);
  if (msg_len == 64u) {
    u64 again[8];
    hmac512_64(again, hm, blk);
    if (memcmp(again, out, sizeof again) != 0) return -2;
  }
  return 0;
}
// the seed (eight 64-bit words) of every line for the passphrase, `rounds` iterations
void bh_seed(const u32* text, const u64* lines, u32 n, const unsigned char* pass, u32 pass_len, u32 rounds, u64* out) {
  bip39_salt salt;
  bip39_salt_block(salt, pass, pass_len);
  for (u32 i = 0; i < n; ++i) bip39_seed(out + (size_t)i * 8, text, (u32)lines[i], (u32)(lines[i] >> 32), salt, rounds);
}
// what k_bip39_master writes: 16 words per line
void bh_master(const u32* text, u32 text_bytes, const u64* lines, u32 n, const unsigned char* pass, u32 pass_len, u32* nodes) {
  bip39_salt salt;
  bip39_salt_block(salt, pass, pass_len);
  for (u32 i = 0; i < n; ++i) bip39_master(nodes + (size_t)i * BIP39_NODE_WORDS, text, text_bytes, lines[i], salt);
}
void bh_master_of_seed(const u64* seed, u32* node) { bip32_master(node, seed); }
int bh_ckd(u32* k, u32* c, u32 index, const u32* px, u32 parity) { return bip32_ckd(k, c, index, px, parity) ? 1 : 0; }
// the validity rules on a planted HMAC result
void bh_master_rule(const u64* I, u32* node) { bip32_master_of(node, I); }
int bh_child_rule(u32* k, u32* c, const u64* I) { return bip32_child_of(k, c, I) ? 1 : 0; }
}

static int fail(const char* what) { return printf("%s failed\n", what), 1; }
// a text of lead + len bytes in a heap block of exactly the size the library gives the device text: ceil(bytes / 4) + 2 words
static u32* text_of(const char* msg, u32 len, u32 lead) {
  u32* text = (u32*)calloc(((size_t)lead + len + 3) / 4 + 2, 4);
  memset(text, 0xA5, lead);
  memcpy((char*)text + lead, msg, len);
  return text;
}
static void hex_of(char* hex, const u64* w, int n) {
  for (int j = 0; j < n; ++j) snprintf(hex + 16 * j, 17, "%016llx", (unsigned long long)w[j]);
}
int main() {
  char hex[129];
  {  // FIPS 180-4's "abc" and the empty message, at the four start alignments
    static const struct { const char* msg; const char* hex; } KAT[] = {
        {"", "cf83e1357eefb8bdf1542850d66d8007d620e4050b5715dc83f4a921d36ce9ce47d0d13c5d85f2b0ff8318d2877eec2f63b931bd47417a81a538327af927da3e"},
        {"abc", "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f"}};
    for (const auto& k : KAT)
      for (u32 lead = 0; lead < 4; ++lead) {
        const u32 len = (u32)strlen(k.msg);
        u32* text = text_of(k.msg, len, lead);
        const u64 line = (u64)lead | (u64)len << 32;
        u64 d[8];
        bh_sha512(text, &line, 1, d);
        free(text);
        hex_of(hex, d, 8);
        if (strcmp(hex, k.hex)) return fail("SHA-512 known answer");
      }
  }
  // every length 0..1100 (9 blocks), then 2000 and 4000, as the last line of the block at the four alignments: the same digest, the same
  // 3-round seed, nothing read outside
  static char msg[4000];
  u32 z = 0x9E3779B9u;
  for (size_t i = 0; i < sizeof msg; ++i) z ^= z << 13, z ^= z >> 17, z ^= z << 5, msg[i] = (char)z;
  for (u32 len = 0; len <= 4000; len = len < 1100 ? len + 1 : len < 2000 ? 2000 : len + 2000) {
    u64 first[16];
    for (u32 lead = 0; lead < 4; ++lead) {
      u32* text = text_of(msg, len, lead);
      const u64 line = (u64)lead | (u64)len << 32;
      u64 got[16];
      bh_sha512(text, &line, 1, got);
      bh_seed(text, &line, 1, (const unsigned char*)"x", 1, 3, got + 8);
      free(text);
      if (lead == 0) memcpy(first, got, sizeof got);
      else if (memcmp(first, got, sizeof got)) return fail("the same line at another alignment");
    }
  }
  {  // BIP39's vector: "abandon" x 11 + "about" with no passphrase and with TREZOR; the master node; m/44'/0'/0' (hardened elements only)
    const char* A = "abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon about";
    const u32 len = (u32)strlen(A);
    u32* text = text_of(A, len, 1);
    const u64 line = 1ull | (u64)len << 32;
    u64 seed[8];
    bh_seed(text, &line, 1, nullptr, 0, BIP39_ROUNDS, seed);
    hex_of(hex, seed, 8);
    if (strncmp(hex, "5eb00bbddcf06908", 16) || strcmp(hex + 120, "ce9e38e4")) return fail("BIP39 seed");
    bh_seed(text, &line, 1, (const unsigned char*)"TREZOR", 6, BIP39_ROUNDS, seed);
    hex_of(hex, seed, 8);
    if (strncmp(hex, "c55257c360c07c72", 16) || strcmp(hex + 120, "e7463b04")) return fail("BIP39 seed with a passphrase");
    u32 node[BIP39_NODE_WORDS];
    bh_master(text, 1 + len, &line, 1, nullptr, 0, node);
    free(text);
    char kh[65];
    for (int w = 0; w < 8; ++w) snprintf(kh + 8 * w, 9, "%08x", node[7 - w]);
    if (strcmp(kh, "1837c1be8e2995ec11cda2b066151be2cfb48adf9e47b151d46adab3a21cdf67")) return fail("master key");
    const u32 none[8] = {0};
    static const u32 ELS[3] = {44u | 1u << 31, 1u << 31, 1u << 31};
    for (u32 el : ELS)
      if (!bh_ckd(node, node + 8, el, none, 0)) return fail("a valid child");
    for (int w = 0; w < 8; ++w) snprintf(kh + 8 * w, 9, "%08x", node[7 - w]);
    if (strcmp(kh, "fe64af825b5b78554c33a28b23085fc082f691b3c712cc1d4e66e133297da87a")) return fail("m/44'/0'/0'");
  }
  {  // the validity rules: I_L = 0 and I_L = n give no master; I_L = n - 1 does; a child with I_L + k = n does not exist
    u64 I[8] = {0, 0, 0, 0, 1, 2, 3, 4};
    u32 node[BIP39_NODE_WORDS];
    bh_master_rule(I, node);
    if (!bip32_is_zero(node)) return fail("I_L = 0");
    I[0] = ~0ull, I[1] = 0xFFFFFFFFFFFFFFFEull, I[2] = 0xBAAEDCE6AF48A03Bull, I[3] = 0xBFD25E8CD0364141ull;
    bh_master_rule(I, node);
    if (!bip32_is_zero(node)) return fail("I_L = n");
    I[3] -= 1;
    bh_master_rule(I, node);
    if (bip32_is_zero(node)) return fail("I_L = n - 1");
    u32 k[8] = {1, 0, 0, 0, 0, 0, 0, 0}, c[8] = {0};
    if (bh_child_rule(k, c, I)) return fail("I_L + k = n");
    k[0] = 2;
    if (!bh_child_rule(k, c, I) || k[0] != 1 || k[7] != 0) return fail("I_L + k = n + 1");
  }
  puts("ok");
  return 0;
}
