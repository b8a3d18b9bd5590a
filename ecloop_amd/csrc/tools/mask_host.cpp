// mask_host.cpp — compiles the mask filter of the DEVICE headers (mask.h) and the host planner (host/mask_plan.h) for the host with g++,
// so that the CPU test-suite can check them without a GPU (tests/test_mask_host.py): the filter on given values, the table check, the
// planner's entries and refusals, and the pattern a hit belongs to.  Built as a shared object for the tests; it has a main of its own
// as well - the filter's edge cases and the planner's grammar, checked against values worked out by hand - so the same code can be built
// as a program under a sanitizer and run directly.  Not part of the product library.
#include "../mask.h"
#include "../../host/mask_plan.h"
#include <stddef.h>
#include <stdio.h>
#include <vector>

extern "C" {
// the device's test of m values against a table of n entries: hit[i] = mask_has.  returns 0, or -1 when the table is not one
// ecl_hip_set_bloom accepts
int mk_test_many(const u32* table, u32 n, const u32* h160, u32 m, u8* hit) {
  if (!mask_table_ok(table, n)) return -1;
  mask_t t;
  memset(&t, 0, sizeof t);
  t.table = table, t.n = n;
  for (u32 i = 0; i < m; ++i) hit[i] = mask_has(t, h160 + (size_t)i * 5) ? 1 : 0;
  return 0;
}
int mk_table_ok(const u32* table, unsigned long long n) { return mask_table_ok(table, n) ? 1 : 0; }
unsigned mk_sizeof_mask_t(void) { return (unsigned)sizeof(mask_t); }
// one pattern -> its entry (ten words) and the digits it fixes: 0, or a PFX_E_ code with the reason in why[320]
int mk_pattern_entry(const char* pattern, int eth, u32* out, u32* digits, char* why) {
  msk_entry e;
  unsigned d = 0;
  const int rc = msk_pattern_entry(pattern, eth, &e, &d, why, 320);
  memcpy(out, &e, sizeof e), *digits = d;
  return rc;
}
static std::vector<const char*> lines_of(std::vector<char>& text) {
  std::vector<const char*> pats;
  for (char* l = strtok(text.data(), "\n"); l; l = strtok(nullptr, "\n")) pats.push_back(l);
  return pats;
}
int mk_list_is_masked(const char* lines) {
  std::vector<char> text(lines, lines + strlen(lines) + 1);
  const std::vector<const char*> pats = lines_of(text);
  return msk_list_is_masked(pats.data(), (uint32_t)pats.size());
}
// patterns (one per line) -> the table (room for 16 entries), entry_of[npat]: the entry count, or a PFX_E_ code
int mk_plan(const char* lines, int eth, u32* table, u32* entry_of, char* why) {
  std::vector<char> text(lines, lines + strlen(lines) + 1);
  const std::vector<const char*> pats = lines_of(text);
  msk_plan p;
  const int rc = msk_plan_make(&p, pats.data(), (uint32_t)pats.size(), eth, why, 320);
  if (rc != PFX_OK) return rc;
  const int n = (int)p.nentry;
  memcpy(table, p.entry, sizeof(msk_entry) * p.nentry);
  memcpy(entry_of, p.entry_of, sizeof(u32) * p.npat);
  msk_plan_free(&p);
  return n;
}
// the first pattern (one per line) the address of h matches, its text in addr[48]; -1: none, -2: the list is refused
int mk_match(const char* lines, int eth, const u32* h, char* addr) {
  std::vector<char> text(lines, lines + strlen(lines) + 1);
  const std::vector<const char*> pats = lines_of(text);
  msk_plan p;
  char why[320];
  if (msk_plan_make(&p, pats.data(), (uint32_t)pats.size(), eth, why, sizeof why) != PFX_OK) return -2;
  const int r = msk_match(&p, h, addr);
  msk_plan_free(&p);
  return r;
}
}

static int fail(const char* what) { return printf("%s failed\n", what), 1; }
static bool has1(const u32* table, u32 n, const u32 h[5]) {
  u8 hit = 2;
  return mk_test_many(table, n, h, 1, &hit) == 0 && hit == 1;
}
int main() {
  if (sizeof(mask_t) != 24) return fail("sizeof(mask_t)");
  const u32 val[5] = {0x01234567u, 0x89abcdefu, 0xdeadbeefu, 0x0badf00du, 0xfeedfaceu};
  // an entry whose only fixed bits lie in one word: a hit, and a miss for each fixed bit flipped
  for (int w = 0; w < 5; ++w) {
    u32 e[10] = {0};
    e[w] = 0x00ffff00u, e[5 + w] = val[w] & 0x00ffff00u;
    if (!has1(e, 1, val)) return fail("one word: hit");
    for (int b = 8; b < 24; ++b) {
      u32 h[5];
      memcpy(h, val, sizeof h);
      h[w] ^= 1u << b;
      if (has1(e, 1, h)) return fail("one word: a flipped fixed bit");
    }
    u32 h[5];  // every bit outside the mask flipped: still a hit
    for (int i = 0; i < 5; ++i) h[i] = ~val[i];
    h[w] = val[w] ^ 0xff0000ffu;
    if (!has1(e, 1, h)) return fail("one word: free bits");
  }
  // the two bits at each word boundary
  for (int w = 0; w < 4; ++w) {
    u32 e[10] = {0};
    e[w] = 1u, e[w + 1] = 0x80000000u, e[5 + w] = val[w] & 1u, e[5 + w + 1] = val[w + 1] & 0x80000000u;
    u32 a[5], b[5];
    memcpy(a, val, sizeof a), memcpy(b, val, sizeof b);
    a[w] ^= 1u, b[w + 1] ^= 0x80000000u;
    if (!has1(e, 1, val) || has1(e, 1, a) || has1(e, 1, b)) return fail("word boundary");
  }
  {  // an all-zero mask matches everything; sixteen entries of which only the last one matches; the table check's refusals
    u32 z[10] = {0}, t[170] = {0};
    if (!has1(z, 1, val)) return fail("all-zero mask");
    for (u32 i = 0; i < 16; ++i) {
      for (int w = 0; w < 5; ++w) t[i * 10 + w] = 0xffffffffu, t[i * 10 + 5 + w] = val[w];
      t[i * 10 + 9] = val[4] ^ (i == 15 ? 0u : (i + 1));
    }
    if (!has1(t, 16, val) || has1(t, 15, val)) return fail("sixteen entries");
    if (mk_table_ok(t, 0) || mk_table_ok(t, 17) || !mk_table_ok(t, 16)) return fail("table check: n");
    u32 stray[10] = {0};
    stray[5] = 1;
    if (mk_table_ok(stray, 1)) return fail("table check: a value bit outside the mask");
    memcpy(t + 10, t, 40);
    if (mk_table_ok(t, 2)) return fail("table check: the same entry twice");
  }
  // the planner: head, tail, both ends, holes, case; the refusals
  char why[320];
  u32 e[10], dg;
  if (mk_pattern_entry("0xdead*beef", 1, e, &dg, why) != PFX_OK || dg != 8 || e[0] != 0xffff0000u || e[5] != 0xdead0000u || e[4] != 0x0000ffffu ||
      e[9] != 0x0000beefu || e[1] | e[2] | e[3] | e[6] | e[7] | e[8])
    return fail("planner: both ends");
  if (mk_pattern_entry("0xDe?d", 1, e, &dg, why) != PFX_OK || dg != 3 || e[0] != 0xff0f0000u || e[5] != 0xde0d0000u) return fail("planner: a hole");
  if (mk_pattern_entry("0x*BEEF?", 1, e, &dg, why) != PFX_OK || dg != 4 || e[4] != 0x000ffff0u || e[9] != 0x000beef0u || e[0]) return fail("planner: a suffix");
  if (mk_pattern_entry("0x0123456789abcdef0123*456789abcdef01234567", 1, e, &dg, why) != PFX_OK || dg != 40 || e[0] != 0xffffffffu || e[5] != 0x01234567u ||
      e[9] != 0x01234567u || e[7] != 0x01234567u)
    return fail("planner: forty digits around the *");
  if (mk_pattern_entry("0xde*ad*", 1, e, &dg, why) != PFX_E_CHAR || !strstr(why, "more than one *")) return fail("planner: two *");
  if (mk_pattern_entry("0xg?", 1, e, &dg, why) != PFX_E_CHAR || !strstr(why, "a character that is no hex digit")) return fail("planner: no hex digit");
  if (mk_pattern_entry("0x??*?", 1, e, &dg, why) != PFX_E_NONE || !strstr(why, "no hex digit at all")) return fail("planner: nothing fixed");
  if (mk_pattern_entry("0x0123456789abcdef0123*456789abcdef012345678", 1, e, &dg, why) != PFX_E_NONE || !strstr(why, "too long")) return fail("planner: too long");
  if (mk_pattern_entry("0xdead*", 0, e, &dg, why) != PFX_E_TYPE || !strstr(why, "a 0x pattern needs -a e")) return fail("planner: without -a e");
  u32 table[160], entry_of[32];
  if (mk_plan("0xdead0*\n0xDEAD0\n0x*beef1\n", 1, table, entry_of, why) != 2 || entry_of[0] != 0 || entry_of[1] != 0 || entry_of[2] != 1) return fail("plan: merged entries");
  if (mk_plan("0xdea*\n", 1, table, entry_of, why) != PFX_E_WIDE || !strstr(why, "lengthen the pattern")) return fail("plan: coverage");
  if (mk_plan("0xdead*\n0x*beef\n", 1, table, entry_of, why) != PFX_E_WIDE) return fail("plan: coverage of two");
  {
    std::vector<char> many;
    for (int i = 0; i < 17; ++i) {
      char l[32];
      snprintf(l, sizeof l, "0x%05x*\n", 0xabc00 + i);
      many.insert(many.end(), l, l + strlen(l));
    }
    many.push_back(0);
    if (mk_plan(many.data(), 1, table, entry_of, why) != PFX_E_MANY || !strstr(why, "split the list")) return fail("plan: seventeen entries");
    many[many.size() - 10] = 0;  // sixteen of five digits each: exactly 2^-16
    if (mk_plan(many.data(), 1, table, entry_of, why) != 16) return fail("plan: sixteen entries");
  }
  char addr[48];
  if (mk_match("0xfffff*\n0x0123?567*face\n0x*dface\n", 1, val, addr) != 1 || strcmp(addr, "0x0123456789abcdefdeadbeef0badf00dfeedface")) return fail("match");
  if (mk_match("0xfffff*\n0x*edfac?f\n", 1, val, addr) != -1) return fail("match: none");
  if (!mk_list_is_masked("0xdead\n0xbe?f\n") || mk_list_is_masked("0xdead\n1Love\n")) return fail("routing");
  puts("ok");
  return 0;
}
