/* mask_plan.h - the planner of Ethereum patterns with wildcards and suffixes (-p 0xdead*beef -a e): patterns -> entries of the mask table
   the device tests (csrc/mask.h), and the pattern a hit belongs to.  Plain C, no GPU; the CLI includes it, tests/test_mask_host.py
   compiles it through csrc/tools/mask_host.cpp, and ecloop_amd/engine.py (mask_table) mirrors it.

   The grammar, after 0x / 0X: hex digits (case ignored), ? (any one digit) and at most one * (any run of digits, none included).
   Without * the pattern is anchored at the start of the address, 1 ... 40 characters; with * the part before it is anchored at the start
   and the part after it at the END, both together 0 ... 40 characters.  An Ethereum address is plain hex - no checksum characters - so a
   digit at position i from the start fixes bits 159 - 4i ... 156 - 4i of the 160-bit value and a digit at position j from the end fixes
   bits 4j + 3 ... 4j: every pattern is one entry (mask, value).  EIP-55 case is not matched.

   Routing (msk_list_is_masked): a list in which no pattern has ? or * is planned by prefix_plan.h exactly as before; if any pattern has
   one, the whole list becomes one mask table and a plain prefix is a head-only entry there.  Identical entries are merged; more than 16
   distinct ones are refused.  Coverage: the sum over the distinct entries of 2^(-4 f), f the entry's hex digits, is an upper bound of the
   union's share of the space; above 2^-16 (prefix_plan.h's bound, for the same reason: records per launch) the list is refused. */
#ifndef ECLOOP_MASK_PLAN_H
#define ECLOOP_MASK_PLAN_H
#include "prefix_plan.h"

#define MSK_MAX_ENTRIES 16u

typedef struct { uint32_t m[5], v[5]; } msk_entry; /* most significant word first: the table's layout */
typedef struct {
  pfx_pattern *pat;   /* the patterns as given */
  uint32_t npat;
  uint32_t *entry_of; /* per pattern: its entry */
  msk_entry entry[MSK_MAX_ENTRIES]; /* distinct, in the order of their first pattern */
  uint32_t nentry;
} msk_plan;

static int msk_hex_digit(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }
/* a 0x pattern with ? or *: what sends a list to the mask table */
static int msk_is_masked(const char *s) { return pfx_form_of(s) == PFX_HEX && strpbrk(s + 2, "?*") != NULL; }
static int msk_list_is_masked(const char *const *patterns, uint32_t npat) {
  for (uint32_t i = 0; i < npat; ++i)
    if (msk_is_masked(patterns[i])) return 1;
  return 0;
}
/* nibble k of the address (0 = the leading digit) takes the value d */
static void msk_fix(msk_entry *e, unsigned k, unsigned d) {
  const unsigned sh = 28 - 4 * (k & 7);
  e->m[k >> 3] |= 0xFu << sh, e->v[k >> 3] |= (uint32_t)d << sh;
}
/* one pattern of a masked list -> its entry and the number of digits it fixes; PFX_OK or a PFX_E_ code with the reason in why */
static int msk_pattern_entry(const char *s, int eth, msk_entry *e, unsigned *digits, char *why, size_t nwhy) {
  const size_t len = strlen(s);
  memset(e, 0, sizeof *e), *digits = 0;
  if (len == 0 || len > PFX_MAX_LEN) return pfx_fail(why, nwhy, PFX_E_NONE, len ? s : "", "no address can start with it (empty or too long)");
  if (pfx_form_of(s) != PFX_HEX) { /* a list with ? or * is a list of 0x patterns: the other forms fail the type check of -a e, or here */
    pfx_range rs[36];
    const int rc = pfx_pattern_ranges(s, 0, 0, eth, rs, why, nwhy);
    return rc < 0 ? rc : pfx_fail(why, nwhy, PFX_E_TYPE, s, "a list with ? or * holds 0x patterns only");
  }
  if (!eth) return pfx_fail(why, nwhy, PFX_E_TYPE, s, "a 0x pattern needs -a e");
  const char *p = s + 2, *star = NULL;
  for (const char *c = p; *c; ++c) {
    if (*c == '*') {
      if (star) return pfx_fail(why, nwhy, PFX_E_CHAR, s, "more than one * (a pattern has one run of free digits at most)");
      star = c;
    } else if (*c != '?' && msk_hex_digit(*c) < 0) {
      return pfx_fail(why, nwhy, PFX_E_CHAR, s, "a character that is no hex digit");
    }
  }
  const unsigned head = (unsigned)(star ? star - p : (s + len) - p), tail = star ? (unsigned)((s + len) - (star + 1)) : 0;
  if (!star && head == 0) return pfx_fail(why, nwhy, PFX_E_NONE, s, "no address can start with it (1 ... 40 hex digits after 0x)");
  if (head + tail > 40) return pfx_fail(why, nwhy, PFX_E_NONE, s, "no address can match it (too long: an address has 40 digits)");
  for (unsigned i = 0; i < head; ++i)
    if (p[i] != '?') msk_fix(e, i, (unsigned)msk_hex_digit(p[i])), ++*digits;
  for (unsigned j = 0; j < tail; ++j) { /* j from the end */
    const char c = s[len - 1 - j];
    if (c != '?') msk_fix(e, 39 - j, (unsigned)msk_hex_digit(c)), ++*digits;
  }
  if (!*digits) return pfx_fail(why, nwhy, PFX_E_NONE, s, "no hex digit at all: every address matches it");
  return PFX_OK;
}

static void msk_plan_free(msk_plan *p) {
  free(p->pat), free(p->entry_of);
  memset(p, 0, sizeof *p);
}
static int msk_plan_make(msk_plan *p, const char *const *patterns, uint32_t npat, int eth, char *why, size_t nwhy) {
  memset(p, 0, sizeof *p);
  if (npat == 0) { snprintf(why, nwhy, "no patterns given"); return PFX_E_NONE; }
  p->pat = (pfx_pattern *)calloc(npat, sizeof(pfx_pattern));
  p->entry_of = (uint32_t *)calloc(npat, sizeof(uint32_t));
  pfx_num total = pfx_small(0);
  for (uint32_t i = 0; i < npat; ++i) {
    msk_entry e;
    unsigned digits;
    const int rc = msk_pattern_entry(patterns[i], eth, &e, &digits, why, nwhy);
    if (rc != PFX_OK) { msk_plan_free(p); return rc; }
    snprintf(p->pat[i].text, sizeof p->pat[i].text, "%s", patterns[i]);
    p->pat[i].form = PFX_HEX;
    uint32_t at = 0;
    while (at < p->nentry && memcmp(&p->entry[at], &e, sizeof e)) ++at;
    if (at == p->nentry) {
      if (p->nentry == MSK_MAX_ENTRIES) {
        snprintf(why, nwhy, "the patterns ('%s', ...) need more than 16 mask entries: split the list", patterns[0]);
        msk_plan_free(p);
        return PFX_E_MANY;
      }
      p->entry[p->nentry++] = e;
      const pfx_num share = pfx_pow2(160 - 4 * digits);
      total = pfx_add(total, &share);
    }
    p->entry_of[i] = at;
  }
  p->npat = npat;
  const pfx_num bound = pfx_pow2(160 - 16);
  if (pfx_cmp(&total, &bound) > 0) {
    snprintf(why, nwhy, "the patterns ('%s'%s) cover more than 2^-16 of all addresses: one launch would report more records than the device keeps; lengthen the pattern",
             p->pat[0].text, npat > 1 ? ", ..." : "");
    msk_plan_free(p);
    return PFX_E_WIDE;
  }
  return PFX_OK;
}

/* does the lower-case text 0x + 40 digits match the pattern (one that msk_pattern_entry accepted)?  By the text, not by the table */
static int msk_text_matches(const char *pattern, const char *addr) {
  const char *p = pattern + 2, *a = addr + 2, *star = strchr(p, '*');
  const size_t head = star ? (size_t)(star - p) : strlen(p), tail = star ? strlen(star + 1) : 0;
  for (size_t i = 0; i < head; ++i)
    if (p[i] != '?' && (p[i] | 0x20) != a[i]) return 0; /* digits and a-f: | 0x20 lowers a letter and keeps a digit */
  for (size_t j = 0; j < tail; ++j)
    if (star[1 + j] != '?' && (star[1 + j] | 0x20) != a[40 - tail + j]) return 0;
  return 1;
}
/* The first pattern, in list order, that the address of h matches; its text goes to addr (48 bytes).  -1: none - on a mask table that is
   an error, not a dropped edge: the device's test is exact */
static int msk_match(const msk_plan *p, const uint32_t h[5], char addr[48]) {
  pfx_address_eth(addr, h);
  for (uint32_t i = 0; i < p->npat; ++i)
    if (msk_text_matches(p->pat[i].text, addr)) return (int)i;
  return -1;
}
#endif
