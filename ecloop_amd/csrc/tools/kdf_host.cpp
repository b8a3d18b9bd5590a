// kdf_host.cpp — compiles the line hashing of the DEVICE header kdf.h (the body of k_raw_scalars_keccak / k_raw_scalars_camp2) for the
// host with g++, so that the CPU test-suite can check the sponge - every length, every start alignment, the flags - without a GPU
// (tests/test_kdf_host.py).  Built as a shared object for the tests; it has a main of its own as well - the known answers, and every
// length at every alignment in a heap buffer that ends with the text's two spare words - so the same code can be built as a program
// under a sanitizer and run directly: a gather that read behind the spare words would be a heap overflow there.  Not part of the
// product library.
#include "../kdf.h"
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" {
// what a launch over the n entries of `lines` writes: out[8 i ..] = the scalar of line i (8 little-endian words), bad[0] / bad[1] the
// kernel's two flags.  kdf = 1 keccak, 2 sha3, 3 camp2 (the field ECL_KDF_* >> 14).  `text` holds text_bytes bytes and two spare words.
void kh_lines(const u32* text, u32 text_bytes, u32 text_have, const u64* lines, u32 n, u32 kdf, u32* out, u32* bad) {
  for (u32 i = 0; i < n; ++i) {
    u32* o = out + (size_t)i * 8;
    if (kdf == 3) kdf_line<KDF_PAD_KECCAK, true>(text, text_bytes, text_have, lines[i], o, bad);
    else if (kdf == 2) kdf_line<KDF_PAD_SHA3, false>(text, text_bytes, text_have, lines[i], o, bad);
    else kdf_line<KDF_PAD_KECCAK, false>(text, text_bytes, text_have, lines[i], o, bad);
  }
}
}

static int fail(const char* what) { return printf("%s failed\n", what), 1; }
// the digest of the `len` bytes at `msg`, hashed as the LAST line of a text of lead + len bytes that lives in a heap block of exactly
// the size the library gives the device text: ceil(bytes / 4) + 2 words.  -> hex (64 digits), or nullptr when a flag was raised
static const char* digest_at(u32 kdf, const char* msg, u32 len, u32 lead) {
  static char hex[65];
  const u32 bytes = lead + len;
  const size_t words = ((size_t)bytes + 3) / 4 + 2;
  u32* text = (u32*)calloc(words, 4);
  memset(text, 0xA5, lead);
  memcpy((char*)text + lead, msg, len);
  const u64 line = (u64)lead | (u64)len << 32;
  u32 out[8], bad[2] = {0, 0};
  kh_lines(text, bytes, bytes, &line, 1, kdf, out, bad);
  free(text);
  if (bad[0] | bad[1]) return nullptr;
  for (int w = 0; w < 8; ++w) snprintf(hex + 8 * w, 9, "%08x", out[7 - w]);
  return hex;
}
int main() {
  static const struct { u32 kdf; const char* msg; const char* hex; } KAT[] = {
      {1, "", "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"},
      {1, "abc", "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"},
      {2, "", "a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a"},
      {2, "abc", "3a985da74fe225b2045c172d6bd390bd855f086e3e9d525b46bfe24511431532"},
      {3, "", "26d412aa8b9fea49149a7dbf8b19672d8813f741842ac1847571d335908cbe65"},
      {3, "abc", "7a44789ed3cd85861c0bbf9693c7e1de1862dd4396c390147ecf1275099c6e6f"},
      {3, "password", "5e225b381fcf02bd5577885f19b9472234c117dc44df6b59aca6690471dea0a0"}};
  for (const auto& k : KAT)
    for (u32 lead = 0; lead < 4; ++lead) {
      const char* got = digest_at(k.kdf, k.msg, (u32)strlen(k.msg), lead);
      if (!got || strcmp(got, k.hex)) return fail("known answer");
    }
  // every length 0..300 and 407, 408, 409, 1000, 4000, ending on the text's last byte, at the four start alignments: the same digest at
  // each (the known answers above say which), nothing read outside the block, no flag
  static char msg[4000];
  u32 z = 0x9E3779B9u;
  for (size_t i = 0; i < sizeof msg; ++i) z ^= z << 13, z ^= z >> 17, z ^= z << 5, msg[i] = (char)z;
  static const u32 MORE[] = {407, 408, 409, 1000, 4000};
  for (u32 kdf = 1; kdf <= 2; ++kdf)
    for (u32 c = 0; c < 301 + 5; ++c) {
      const u32 len = c < 301 ? c : MORE[c - 301];
      char first[65];
      for (u32 lead = 0; lead < 4; ++lead) {
        const char* got = digest_at(kdf, msg, len, lead);
        if (!got) return fail("a flag for a line inside the text");
        if (lead == 0) memcpy(first, got, 65);
        else if (strcmp(first, got)) return fail("the same line at another alignment");
      }
    }
  {  // a line that ends one byte behind the text: flag [0], nothing read; a line behind what is on the device: flag [1]
    u32* text = (u32*)calloc((10 + 3) / 4 + 2, 4);
    memcpy(text, "0123456789", 10);
    const u64 lines[2] = {8ull | 3ull << 32, 6ull | 4ull << 32};
    u32 out[16], bad[2] = {0, 0};
    kh_lines(text, 10, 10, lines, 1, 1, out, bad);
    if (bad[0] != 1 || bad[1] != 0) return fail("flag [0]");
    bad[0] = 0;
    kh_lines(text, 10, 8, lines + 1, 1, 1, out, bad);
    free(text);
    if (bad[0] != 0 || bad[1] != 1) return fail("flag [1]");
  }
  puts("ok");
  return 0;
}
