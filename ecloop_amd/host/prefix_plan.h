/* prefix_plan.h - the planner of the prefix search (-p): address patterns -> inclusive ranges over the 160-bit value the device tests
   (csrc/prefix.h), and the address text of a hit.  Plain C, no GPU; the CLI includes it, tests/test_prefix_host.py compiles it through
   csrc/tools/prefix_host.cpp, and ecloop_amd/engine.py (prefix_ranges) mirrors it.

   Three pattern forms:
     1...     base58 P2PKH (-a c, u or cu).  An address is base58check(00 || hash160): k leading '1's are k zero bytes in front - the
              version byte and k - 1 leading zero bytes of the hash - and the rest is the base58 number N of the other bytes, hash and
              checksum together (N = hash160 * 2^32 + checksum).  A pattern of k '1's and m more digits of value v: for every digit count D
              that N can have, N lies in [v 58^(D-m), (v + 1) 58^(D-m) - 1], clipped to the numbers of exactly 24 - (k - 1) bytes; shifted
              right by 32 bits that is a range of the hash.  Conservative at a range's two end values, where only some checksums fit: the
              caller encodes every hit and compares the text.  A pattern of '1's alone: the hashes with at least k - 1 leading zero bytes.
     bc1q...  bech32 P2WPKH (-a c only): each character after the q is five leading bits of the hash, 32 characters at most; lower case,
              or all upper case.
     0x...    Ethereum (-a e): each hex digit is four leading bits, 40 digits at most; case is ignored (EIP-55 case is not matched).
   Ranges of several patterns are merged where they overlap or touch; every merged range keeps the patterns it serves.  Patterns that
   together cover more than 2^-16 of the space are refused: at twelve hashes per key (-a cu -endo) a 2^32-key launch then reports about
   2^19.6 records, inside the 2^20 the device keeps per call.  The fraction is computed, not guessed from the length: base58 leading digits
   are far from uniform (1Q covers 2^-6, 1z covers 2^-10.4). */
#ifndef ECLOOP_PREFIX_PLAN_H
#define ECLOOP_PREFIX_PLAN_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define PFX_MAX_LEN 44      /* longest pattern text kept (0x + 40 digits) */
#define PFX_MAX_RANGES 65536u
enum { PFX_B58 = 1, PFX_BECH32 = 2, PFX_HEX = 3 };
enum { PFX_OK = 0, PFX_E_CHAR = -1, PFX_E_NONE = -2, PFX_E_TYPE = -3, PFX_E_UNSUPPORTED = -4, PFX_E_WIDE = -5, PFX_E_MANY = -6 };

typedef struct { uint32_t w[8]; } pfx_num; /* 256 bits, little-endian words */
typedef struct { uint32_t lo[5], hi[5]; } pfx_range; /* most significant word first: the table's layout */
typedef struct { char text[PFX_MAX_LEN + 1]; int form; } pfx_pattern;
typedef struct {
  pfx_pattern *pat;
  uint32_t npat;
  pfx_range *range;   /* merged, sorted by lo, disjoint and not adjacent */
  uint32_t nrange;
  uint32_t *serve_at; /* nrange + 1 offsets into serve */
  uint32_t *serve;    /* the patterns each range serves, ascending */
} pfx_plan;

static const char PFX_B58_ALPHABET[] = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";
static const char PFX_BECH32_ALPHABET[] = "qpzry9x8gf2tvdw0s3jn54khce6mua7l";

/* ---- 256-bit helpers */
static pfx_num pfx_small(uint32_t v) { pfx_num r; memset(&r, 0, sizeof r); r.w[0] = v; return r; }
static pfx_num pfx_pow2(unsigned e) { pfx_num r; memset(&r, 0, sizeof r); r.w[e >> 5] = 1u << (e & 31); return r; }
static int pfx_cmp(const pfx_num *a, const pfx_num *b) {
  for (int i = 7; i >= 0; --i)
    if (a->w[i] != b->w[i]) return a->w[i] > b->w[i] ? 1 : -1;
  return 0;
}
static pfx_num pfx_muladd(pfx_num a, uint32_t m, uint32_t c) { /* a * m + c (the callers stay below 2^256) */
  uint64_t carry = c;
  for (int i = 0; i < 8; ++i) carry += (uint64_t)a.w[i] * m, a.w[i] = (uint32_t)carry, carry >>= 32;
  return a;
}
static pfx_num pfx_add(pfx_num a, const pfx_num *b) {
  uint64_t c = 0;
  for (int i = 0; i < 8; ++i) c += (uint64_t)a.w[i] + b->w[i], a.w[i] = (uint32_t)c, c >>= 32;
  return a;
}
static pfx_num pfx_sub(pfx_num a, const pfx_num *b) {
  uint64_t br = 0;
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)a.w[i] - b->w[i] - br;
    a.w[i] = (uint32_t)d, br = (d >> 32) & 1;
  }
  return a;
}
static pfx_num pfx_shr32(pfx_num a) {
  for (int i = 0; i < 7; ++i) a.w[i] = a.w[i + 1];
  a.w[7] = 0;
  return a;
}
static void pfx_to_words5(uint32_t out[5], const pfx_num *a) { for (int i = 0; i < 5; ++i) out[i] = a->w[4 - i]; }
static pfx_num pfx_from_words5(const uint32_t in[5]) {
  pfx_num r;
  memset(&r, 0, sizeof r);
  for (int i = 0; i < 5; ++i) r.w[4 - i] = in[i];
  return r;
}

/* ---- one pattern -> its ranges (at most 36); returns the count or a PFX_E_ code, with the reason in why */
static int pfx_index_of(const char *alphabet, char c) {
  const char *p = c ? strchr(alphabet, c) : NULL;
  return p ? (int)(p - alphabet) : -1;
}
static int pfx_fail(char *why, size_t n, int code, const char *pattern, const char *reason) {
  snprintf(why, n, "pattern '%s': %s", pattern, reason);
  return code;
}
static int pfx_form_of(const char *s) {
  if (s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) return PFX_HEX;
  if ((!strncmp(s, "bc1q", 4)) || (!strncmp(s, "BC1Q", 4))) return PFX_BECH32;
  if (s[0] == '1') return PFX_B58;
  return 0;
}
/* leading `bits` bits of the 160 given in v (right-aligned): the range of the hashes that start with them */
static void pfx_bits_range(pfx_range *r, const pfx_num *v, unsigned bits) {
  pfx_num lo = *v, ones = pfx_pow2(160 - bits), one = pfx_small(1);
  for (unsigned i = bits; i < 160; ++i) lo = pfx_add(lo, &lo);
  ones = pfx_sub(ones, &one);
  const pfx_num hi = pfx_add(lo, &ones);
  pfx_to_words5(r->lo, &lo), pfx_to_words5(r->hi, &hi);
}
static int pfx_pattern_ranges(const char *s, int a33, int a65, int eth, pfx_range out[36], char *why, size_t nwhy) {
  const size_t len = strlen(s);
  const int form = pfx_form_of(s);
  if (len == 0 || len > PFX_MAX_LEN) return pfx_fail(why, nwhy, PFX_E_NONE, len ? s : "", "no address can start with it (empty or too long)");
  if (!form) {
    if (s[0] == '3') return pfx_fail(why, nwhy, PFX_E_UNSUPPORTED, s, "P2SH patterns (3...) are not supported yet");
    if (!strncmp(s, "bc1p", 4) || !strncmp(s, "BC1P", 4)) return pfx_fail(why, nwhy, PFX_E_UNSUPPORTED, s, "Taproot patterns (bc1p...) are not supported yet");
    if (strspn(s, "0123456789abcdefABCDEF") == len) return pfx_fail(why, nwhy, PFX_E_UNSUPPORTED, s, "bare hex patterns are not supported yet (an Ethereum pattern starts with 0x)");
    return pfx_fail(why, nwhy, PFX_E_NONE, s, "no address can start with it (patterns start with 1, bc1q or 0x)");
  }
  if (form == PFX_HEX) {
    if (!eth) return pfx_fail(why, nwhy, PFX_E_TYPE, s, "a 0x pattern needs -a e");
    const unsigned nd = (unsigned)len - 2;
    if (nd == 0 || nd > 40) return pfx_fail(why, nwhy, PFX_E_NONE, s, "no address can start with it (1 ... 40 hex digits after 0x)");
    pfx_num v = pfx_small(0);
    for (unsigned i = 0; i < nd; ++i) {
      const char c = s[2 + i];
      const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
      if (d < 0) return pfx_fail(why, nwhy, PFX_E_CHAR, s, "a character that is no hex digit");
      v = pfx_muladd(v, 16, (uint32_t)d);
    }
    pfx_bits_range(&out[0], &v, 4 * nd);
    return 1;
  }
  if (form == PFX_BECH32) {
    if (eth || !a33 || a65) return pfx_fail(why, nwhy, PFX_E_TYPE, s, "a bc1q pattern needs -a c (P2WPKH is the compressed key's hash alone)");
    const unsigned nd = (unsigned)len - 4;
    const int upper = s[0] == 'B';
    if (nd == 0 || nd > 32) return pfx_fail(why, nwhy, PFX_E_NONE, s, "no address can start with it (1 ... 32 characters after bc1q)");
    pfx_num v = pfx_small(0);
    for (unsigned i = 0; i < nd; ++i) {
      char c = s[4 + i];
      if (upper && c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
      else if (upper ? (c >= 'a' && c <= 'z') : (c >= 'A' && c <= 'Z')) return pfx_fail(why, nwhy, PFX_E_CHAR, s, "mixed case (bech32 is lower case, or all upper case)");
      const int d = pfx_index_of(PFX_BECH32_ALPHABET, c);
      if (d < 0) return pfx_fail(why, nwhy, PFX_E_CHAR, s, "a character outside the bech32 alphabet (it has no 1, b, i, o)");
      v = pfx_muladd(v, 32, (uint32_t)d);
    }
    pfx_bits_range(&out[0], &v, 5 * nd);
    return 1;
  }
  /* base58 */
  if (eth || (!a33 && !a65)) return pfx_fail(why, nwhy, PFX_E_TYPE, s, "a 1... pattern needs -a c, u or cu");
  for (size_t i = 0; i < len; ++i)
    if (pfx_index_of(PFX_B58_ALPHABET, s[i]) < 0) return pfx_fail(why, nwhy, PFX_E_CHAR, s, "a character outside the base58 alphabet (it has no 0, O, I, l)");
  unsigned k = 0;
  while (s[k] == '1') ++k;
  const unsigned z = k - 1, m = (unsigned)len - k; /* zero bytes of the hash, digits of v */
  if (z > 20) return pfx_fail(why, nwhy, PFX_E_NONE, s, "no address can start with it (more leading 1s than a hash has zero bytes)");
  if (m == 0) { /* at least z leading zero bytes */
    const pfx_num zero = pfx_small(0);
    if (z == 20) { pfx_to_words5(out[0].lo, &zero), pfx_to_words5(out[0].hi, &zero); return 1; }
    pfx_bits_range(&out[0], &zero, 8 * z);
    return 1;
  }
  if (m > 33) return pfx_fail(why, nwhy, PFX_E_NONE, s, "no address can start with it (too long)");
  pfx_num v = pfx_small(0), one = pfx_small(1);
  for (unsigned i = 0; i < m; ++i) v = pfx_muladd(v, 58, (uint32_t)pfx_index_of(PFX_B58_ALPHABET, s[k + i]));
  /* the numbers of exactly L = 24 - z bytes: [2^(8(L-1)), 2^(8L) - 1] */
  const unsigned L = 24 - z;
  const pfx_num bmin = pfx_pow2(8 * (L - 1));
  pfx_num bmax = pfx_pow2(8 * L);
  bmax = pfx_sub(bmax, &one);
  int n = 0;
  pfx_num lo = v, hi1 = pfx_muladd(v, 1, 1); /* v 58^(D-m) and (v + 1) 58^(D-m) for D = m, m + 1, ... */
  for (unsigned D = m; D <= 33; ++D) {
    if (pfx_cmp(&lo, &bmax) > 0) break;
    pfx_num a = lo, b = pfx_sub(hi1, &one);
    if (pfx_cmp(&b, &bmin) >= 0) {
      if (pfx_cmp(&a, &bmin) < 0) a = bmin;
      if (pfx_cmp(&b, &bmax) > 0) b = bmax;
      a = pfx_shr32(a), b = pfx_shr32(b);
      pfx_to_words5(out[n].lo, &a), pfx_to_words5(out[n].hi, &b);
      ++n;
    }
    lo = pfx_muladd(lo, 58, 0), hi1 = pfx_muladd(hi1, 58, 0); /* below 58^34 < 2^200 */
  }
  if (!n) return pfx_fail(why, nwhy, PFX_E_NONE, s, "no address can start with it (no hash gives these leading digits)");
  return n;
}

/* ---- the plan of several patterns */
typedef struct { pfx_range r; uint32_t pat; } pfx_item;
static int pfx_item_order(const void *a, const void *b) {
  const pfx_item *x = (const pfx_item *)a, *y = (const pfx_item *)b;
  for (int i = 0; i < 5; ++i) /* (word by word: memcmp would compare bytes) */
    if (x->r.lo[i] != y->r.lo[i]) return x->r.lo[i] > y->r.lo[i] ? 1 : -1;
  return (x->pat > y->pat) - (x->pat < y->pat);
}
static void pfx_plan_free(pfx_plan *p) {
  free(p->pat), free(p->range), free(p->serve_at), free(p->serve);
  memset(p, 0, sizeof *p);
}
static int pfx_plan_make(pfx_plan *p, const char *const *patterns, uint32_t npat, int a33, int a65, int eth, char *why, size_t nwhy) {
  memset(p, 0, sizeof *p);
  if (npat == 0) { snprintf(why, nwhy, "no patterns given"); return PFX_E_NONE; }
  pfx_item *items = (pfx_item *)malloc(sizeof(pfx_item) * 36 * (size_t)npat);
  p->pat = (pfx_pattern *)calloc(npat, sizeof(pfx_pattern));
  uint32_t nitems = 0;
  for (uint32_t i = 0; i < npat; ++i) {
    pfx_range rs[36];
    const int n = pfx_pattern_ranges(patterns[i], a33, a65, eth, rs, why, nwhy);
    if (n < 0) { free(items), pfx_plan_free(p); return n; }
    snprintf(p->pat[i].text, sizeof p->pat[i].text, "%s", patterns[i]);
    p->pat[i].form = pfx_form_of(patterns[i]);
    for (int j = 0; j < n; ++j) items[nitems].r = rs[j], items[nitems].pat = i, ++nitems;
  }
  p->npat = npat;
  qsort(items, nitems, sizeof *items, pfx_item_order);
  p->range = (pfx_range *)malloc(sizeof(pfx_range) * nitems);
  p->serve_at = (uint32_t *)malloc(sizeof(uint32_t) * (nitems + 1));
  p->serve = (uint32_t *)malloc(sizeof(uint32_t) * nitems);
  uint32_t nserve = 0;
  pfx_num total = pfx_small(0), one = pfx_small(1);
  for (uint32_t i = 0; i < nitems;) { /* merge what overlaps or touches */
    pfx_num lo = pfx_from_words5(items[i].r.lo), hi = pfx_from_words5(items[i].r.hi);
    p->serve_at[p->nrange] = nserve;
    uint32_t j = i;
    for (; j < nitems; ++j) {
      const pfx_num l = pfx_from_words5(items[j].r.lo), h = pfx_from_words5(items[j].r.hi), next = pfx_add(hi, &one);
      if (j > i && pfx_cmp(&l, &next) > 0) break;
      if (pfx_cmp(&h, &hi) > 0) hi = h;
      uint32_t at = p->serve_at[p->nrange]; /* the served patterns, ascending and unique */
      while (at < nserve && p->serve[at] < items[j].pat) ++at;
      if (at == nserve || p->serve[at] != items[j].pat) {
        memmove(p->serve + at + 1, p->serve + at, sizeof(uint32_t) * (nserve - at));
        p->serve[at] = items[j].pat, ++nserve;
      }
    }
    pfx_to_words5(p->range[p->nrange].lo, &lo), pfx_to_words5(p->range[p->nrange].hi, &hi);
    const pfx_num size = pfx_add(pfx_sub(hi, &lo), &one);
    total = pfx_add(total, &size);
    ++p->nrange, i = j;
  }
  p->serve_at[p->nrange] = nserve;
  free(items);
  const pfx_num bound = pfx_pow2(160 - 16);
  if (pfx_cmp(&total, &bound) > 0) {
    snprintf(why, nwhy, "the patterns ('%s'%s) cover more than 2^-16 of all addresses: one launch would report more records than the device keeps; lengthen the pattern",
             p->pat[0].text, npat > 1 ? ", ..." : "");
    pfx_plan_free(p);
    return PFX_E_WIDE;
  }
  if (p->nrange > PFX_MAX_RANGES) {
    snprintf(why, nwhy, "the patterns need more than 65536 ranges");
    pfx_plan_free(p);
    return PFX_E_MANY;
  }
  return PFX_OK;
}

/* ---- SHA-256 (FIPS 180-4), for the checksum of a base58check address */
static uint32_t pfx_rotr(uint32_t x, int n) { return x >> n | x << (32 - n); }
static void pfx_sha256(uint8_t out[32], const uint8_t *msg, size_t len) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
      0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
      0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
      0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
      0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
      0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  const size_t total = (len + 9 + 63) / 64 * 64;
  for (size_t at = 0; at < total; at += 64) {
    uint8_t blk[64];
    for (size_t i = 0; i < 64; ++i) {
      const size_t p = at + i;
      blk[i] = p < len ? msg[p] : p == len ? 0x80 : p >= total - 8 ? (uint8_t)(((uint64_t)len * 8) >> (8 * (total - 1 - p))) : 0;
    }
    uint32_t w[64], s[8];
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)blk[4 * i] << 24 | (uint32_t)blk[4 * i + 1] << 16 | (uint32_t)blk[4 * i + 2] << 8 | blk[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = pfx_rotr(w[i - 15], 7) ^ pfx_rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
      const uint32_t s1 = pfx_rotr(w[i - 2], 17) ^ pfx_rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    memcpy(s, h, sizeof s);
    for (int i = 0; i < 64; ++i) {
      const uint32_t S1 = pfx_rotr(s[4], 6) ^ pfx_rotr(s[4], 11) ^ pfx_rotr(s[4], 25), ch = (s[4] & s[5]) ^ (~s[4] & s[6]);
      const uint32_t t1 = s[7] + S1 + ch + K[i] + w[i];
      const uint32_t S0 = pfx_rotr(s[0], 2) ^ pfx_rotr(s[0], 13) ^ pfx_rotr(s[0], 22), maj = (s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]);
      const uint32_t t2 = S0 + maj;
      s[7] = s[6], s[6] = s[5], s[5] = s[4], s[4] = s[3] + t1, s[3] = s[2], s[2] = s[1], s[1] = s[0], s[0] = t1 + t2;
    }
    for (int i = 0; i < 8; ++i) h[i] += s[i];
  }
  for (int i = 0; i < 8; ++i) out[4 * i] = (uint8_t)(h[i] >> 24), out[4 * i + 1] = (uint8_t)(h[i] >> 16), out[4 * i + 2] = (uint8_t)(h[i] >> 8), out[4 * i + 3] = (uint8_t)h[i];
}

/* ---- the address text of a hash (h: five words, most significant first) */
static void pfx_bytes_of(uint8_t b[20], const uint32_t h[5]) {
  for (int i = 0; i < 20; ++i) b[i] = (uint8_t)(h[i >> 2] >> (8 * (3 - (i & 3))));
}
static void pfx_address_b58(char out[40], const uint32_t h[5]) { /* base58check(00 || hash) */
  uint8_t raw[25], d1[32], d2[32];
  raw[0] = 0;
  pfx_bytes_of(raw + 1, h);
  pfx_sha256(d1, raw, 21), pfx_sha256(d2, d1, 32);
  memcpy(raw + 21, d2, 4);
  int zeros = 0;
  while (zeros < 25 && raw[zeros] == 0) ++zeros;
  char digits[40];
  int nd = 0;
  uint8_t num[25];
  memcpy(num, raw, 25);
  for (;;) { /* divide the 25-byte number by 58 until it is zero */
    unsigned rem = 0;
    int any = 0;
    for (int i = 0; i < 25; ++i) {
      const unsigned cur = rem * 256 + num[i];
      num[i] = (uint8_t)(cur / 58), rem = cur % 58;
      any |= num[i];
    }
    digits[nd++] = PFX_B58_ALPHABET[rem];
    if (!any) break;
  }
  if (nd == 1 && digits[0] == '1') nd = 0; /* the number was zero: the leading-zero rule writes its bytes */
  int at = 0;
  for (int i = 0; i < zeros; ++i) out[at++] = '1';
  while (nd) out[at++] = digits[--nd];
  out[at] = 0;
}
static uint32_t pfx_bech32_polymod(const uint8_t *v, size_t n) {
  static const uint32_t GEN[5] = {0x3b6a57b2, 0x26508e6d, 0x1ea119fa, 0x3d4233dd, 0x2a1462b3};
  uint32_t chk = 1;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t b = chk >> 25;
    chk = (chk & 0x1ffffff) << 5 ^ v[i];
    for (int j = 0; j < 5; ++j)
      if ((b >> j) & 1) chk ^= GEN[j];
  }
  return chk;
}
static void pfx_address_bech32(char out[48], const uint32_t h[5], int upper) { /* BIP173: hrp bc, witness version 0, the 20-byte program */
  uint8_t b[20], v[5 + 1 + 32 + 6] = {3, 3, 0, 2, 3, 0}; /* hrp expanded: b >> 5, c >> 5, 0, b & 31, c & 31; then the version */
  pfx_bytes_of(b, h);
  for (int i = 0; i < 32; ++i) { /* 160 bits in groups of five */
    const int bit = 5 * i;
    const unsigned two = (unsigned)b[bit >> 3] << 8 | (bit / 8 + 1 < 20 ? b[bit / 8 + 1] : 0);
    v[6 + i] = (uint8_t)((two >> (11 - (bit & 7))) & 31);
  }
  memset(v + 38, 0, 6);
  const uint32_t pm = pfx_bech32_polymod(v, sizeof v) ^ 1;
  for (int i = 0; i < 6; ++i) v[38 + i] = (uint8_t)((pm >> (5 * (5 - i))) & 31);
  memcpy(out, "bc1", 3);
  for (int i = 0; i < 39; ++i) out[3 + i] = PFX_BECH32_ALPHABET[v[5 + i]];
  out[42] = 0;
  if (upper)
    for (int i = 0; i < 42; ++i)
      if (out[i] >= 'a' && out[i] <= 'z') out[i] = (char)(out[i] - 'a' + 'A');
}
static void pfx_address_eth(char out[48], const uint32_t h[5]) {
  snprintf(out, 48, "0x%08x%08x%08x%08x%08x", h[0], h[1], h[2], h[3], h[4]);
}
/* The first pattern, in list order, that the address of h (record type: 1 addr33, 0 addr65, 3 eth) starts with; its address text, in that
   pattern's form, goes to addr (48 bytes).  -1: none - a range's end value whose checksum does not fit.  A hex pattern is compared without
   regard to case. */
static int pfx_match(const pfx_plan *p, const uint32_t h[5], int type, char addr[48]) {
  char b58[48] = "", bech[48] = "", hex[48] = "";
  for (uint32_t i = 0; i < p->npat; ++i) {
    const pfx_pattern *q = &p->pat[i];
    const size_t n = strlen(q->text);
    if (q->form == PFX_HEX && type == 3) {
      if (!hex[0]) pfx_address_eth(hex, h);
      size_t k = 2;
      while (k < n && (q->text[k] | 0x20) == hex[k]) ++k; /* digits and a-f: | 0x20 lowers a letter and keeps a digit */
      if (k == n) { strcpy(addr, hex); return (int)i; }
    } else if (q->form == PFX_BECH32 && type == 1) {
      const int upper = q->text[0] == 'B';
      pfx_address_bech32(bech, h, upper);
      if (!strncmp(bech, q->text, n)) { strcpy(addr, bech); return (int)i; }
    } else if (q->form == PFX_B58 && (type == 0 || type == 1)) {
      if (!b58[0]) pfx_address_b58(b58, h);
      if (!strncmp(b58, q->text, n)) { strcpy(addr, b58); return (int)i; }
    }
  }
  return -1;
}
#endif
