// prefix_host.cpp — compiles the prefix filter of the DEVICE headers (prefix.h) and the host planner (host/prefix_plan.h) for the host with
// g++, so that the CPU test-suite can check them without a GPU (tests/test_prefix_host.py): the two stages of the filter on given values,
// the table check and the bitmap ecl_hip_set_bloom builds, the planner's ranges and the address text of a hit.  Built as a shared object
// for the tests; it has a main of its own as well (a short self-check), so the same code can be built as a program under a sanitizer and
// run directly.  Not part of the product library.
#include "../prefix.h"
#include "../../host/prefix_plan.h"
#include <stddef.h>
#include <stdio.h>
#include <vector>

extern "C" {
// the device's two-stage test of m values against a table of n ranges: stage1[i] = the bitmap's bit, hit[i] = prefix_has.
// returns 0, or -1 when the table is not one ecl_hip_set_bloom accepts
int px_test_many(const u32* table, u32 n, const u32* h160, u32 m, u8* stage1, u8* hit) {
  if (!prefix_table_ok(table, n)) return -1;
  const u32 shift = 32u - PREFIX_BUCKET_BITS;
  std::vector<u32> bitmap(((size_t)1 << PREFIX_BUCKET_BITS) / 32u);
  prefix_build_bitmap(bitmap.data(), table, n, shift);
  prefix_t p;
  p.bitmap = bitmap.data(), p.table = table, p.n = n, p.shift = shift;
  for (u32 i = 0; i < m; ++i) {
    stage1[i] = prefix_stage1(p, h160 + (size_t)i * 5) ? 1 : 0;
    hit[i] = prefix_has(p, h160 + (size_t)i * 5) ? 1 : 0;
  }
  return 0;
}
int px_table_ok(const u32* table, unsigned long long n) { return prefix_table_ok(table, n) ? 1 : 0; }
// number of set bits of the bitmap of a table (a bucket's bit is set iff a range intersects it)
unsigned long long px_bitmap_popcount(const u32* table, u32 n) {
  std::vector<u32> bitmap(((size_t)1 << PREFIX_BUCKET_BITS) / 32u);
  prefix_build_bitmap(bitmap.data(), table, n, 32u - PREFIX_BUCKET_BITS);
  unsigned long long c = 0;
  for (u32 w : bitmap) c += (unsigned)__builtin_popcount(w);
  return c;
}
// one pattern -> its ranges before merging (ten words each, room for 36): the count, or a PFX_E_ code with the reason in why[320]
int px_pattern_ranges(const char* pattern, int a33, int a65, int eth, u32* out, char* why) {
  pfx_range rs[36];
  const int n = pfx_pattern_ranges(pattern, a33, a65, eth, rs, why, 320);
  if (n > 0) memcpy(out, rs, sizeof(pfx_range) * (size_t)n);
  return n;
}
// patterns (one per line) -> the merged table (room for cap ranges), serve_at[nrange + 1], serve[]: the range count, or a PFX_E_ code
int px_plan(const char* lines, int a33, int a65, int eth, u32* table, u32 cap, u32* serve_at, u32* serve, char* why) {
  std::vector<char> text(lines, lines + strlen(lines) + 1);
  std::vector<const char*> pats;
  for (char* l = strtok(text.data(), "\n"); l; l = strtok(nullptr, "\n")) pats.push_back(l);
  pfx_plan p;
  const int rc = pfx_plan_make(&p, pats.data(), (uint32_t)pats.size(), a33, a65, eth, why, 320);
  if (rc != PFX_OK) return rc;
  const int n = (int)p.nrange;
  if (p.nrange <= cap) {
    memcpy(table, p.range, sizeof(pfx_range) * p.nrange);
    memcpy(serve_at, p.serve_at, sizeof(u32) * (p.nrange + 1));
    memcpy(serve, p.serve, sizeof(u32) * p.serve_at[p.nrange]);
  }
  pfx_plan_free(&p);
  return n;
}
// the address text of a hash: form 1 base58, 2 bech32 (upper: all upper case), 3 Ethereum; out[48]
void px_address(const u32* h, int form, int upper, char* out) {
  if (form == PFX_B58) pfx_address_b58(out, h);
  else if (form == PFX_BECH32) pfx_address_bech32(out, h, upper);
  else pfx_address_eth(out, h);
}
// the first pattern (one per line) the record's address starts with, its text in addr[48]; -1: none
int px_match(const char* lines, int a33, int a65, int eth, const u32* h, int type, char* addr) {
  std::vector<char> text(lines, lines + strlen(lines) + 1);
  std::vector<const char*> pats;
  for (char* l = strtok(text.data(), "\n"); l; l = strtok(nullptr, "\n")) pats.push_back(l);
  pfx_plan p;
  char why[320];
  if (pfx_plan_make(&p, pats.data(), (uint32_t)pats.size(), a33, a65, eth, why, sizeof why) != PFX_OK) return -2;
  const int r = pfx_match(&p, h, type, addr);
  pfx_plan_free(&p);
  return r;
}
void px_sha256(const unsigned char* msg, size_t len, unsigned char* out) { pfx_sha256(out, msg, len); }
}

int main() {
  // SHA-256("abc"), the address of the key 1, a two-range table around a bucket boundary
  unsigned char d[32];
  pfx_sha256(d, (const unsigned char*)"abc", 3);
  if (d[0] != 0xba || d[31] != 0xad) return puts("sha256 failed"), 1;
  const u32 h1[5] = {0x751e76e8u, 0x199196d4u, 0x54941c45u, 0xd1b3a323u, 0xf1433bd6u};
  char a[48];
  pfx_address_b58(a, h1);
  if (strcmp(a, "1BgGZ9tcN4rm9KBzDn7KprQz87SZ26SAMH")) return puts("base58 failed"), 1;
  pfx_address_bech32(a, h1, 0);
  if (strcmp(a, "bc1qw508d6qejxtdg4y5r3zarvary0c5xw7kv8f3t4")) return puts("bech32 failed"), 1;
  const u32 table[20] = {0x000000ffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xfffffff0u, 0x00000100u, 0, 0, 0, 5,
                         0x00000100u, 0, 0, 0, 7, 0x00000100u, 0, 0, 0, 7};
  const u32 vals[4 * 5] = {0x000000ffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffefu, 0x00000100u, 0, 0, 0, 5,
                           0x00000100u, 0, 0, 0, 6, 0x00000100u, 0, 0, 0, 7};
  u8 s1[4], hit[4];
  if (px_test_many(table, 2, vals, 4, s1, hit) != 0 || hit[0] != 0 || hit[1] != 1 || hit[2] != 0 || hit[3] != 1) return puts("filter failed"), 1;
  char why[320];
  u32 out[360];
  if (px_pattern_ranges("1QLbz7", 1, 0, 0, out, why) != 2 || px_pattern_ranges("1l", 1, 0, 0, out, why) != PFX_E_CHAR) return puts("planner failed"), 1;
  puts("ok");
  return 0;
}
