/* gen_plan.h - the template of the `brain` command: pass phrases that are generated where they are hashed.  Plain C, no GPU: the library
   (csrc/abi_gen.h), the CLI (cli_brain.h) and the host test program (csrc/tools/gen_host.cpp) all include this file, so the code that is
   tested is the code that runs.  THIS FILE IS THE DEFINITION of the template; the device's expansion (csrc/gen.h), engine.py and
   tests/brain_ref.py agree with it byte for byte.

   The template.  P positions, 1 <= P <= 16.  Position p has c_p >= 1 alternatives, each a byte string of 0 ... 255 bytes.  L = the sum
   over the positions of the longest alternative, at most 256.  At most 2^22 alternatives and 2^28 bytes of them in all.  T = the product
   of the c_p, below 2^64.  Candidate i, 0 <= i < T, has the digits d_p with i = sum d_p * prod_{q > p} c_q - the LAST position runs
   fastest - and its text is alt[0][d_0] || ... || alt[P - 1][d_{P - 1}].  A literal is a position with one alternative, a character
   class a position of one-byte alternatives, a dictionary a position of words: mask, dictionary, combinator and hybrid attacks are
   this one scheme.

   The blob (what ecl_hip_mul_batch_raw takes as `text` on an ECL_GEN context), packed, little-endian:
       u8 magic[4] = "GEN\0";  u8 npos;  u8 zero[3];  u32 nalt;  u32 pool_bytes;
       { u32 count; u32 first; } pos[npos]     first = index of the position's first alternative: positions in order, contiguous
       { u32 off;  u32 len;   } alt[nalt]      off into the pool
       u8 pool[pool_bytes]
   Alternatives may share bytes of the pool.

   The mask of the command line (gen_parse_mask): ?l a-z, ?u A-Z, ?d 0-9, ?h 0-9a-f, ?s the 33 printable ASCII specials in ASCII order
   (the space first), ?a = ?l?u?d?s in that order (95), ?1 ... ?4 the custom sets, ?? a literal '?'; any other byte is a literal and a run
   of literals is one position.  A custom set (gen_parse_set) is literal bytes and the classes above - one-byte alternatives in the order
   given, a repeated byte refused - or @file: every line of the file an alternative, cut as `mul -raw` cuts lines ('\r' before the
   newline dropped, empty lines skipped, duplicates kept). */
#ifndef GEN_PLAN_H
#define GEN_PLAN_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define GEN_POS_MAX 16u
#define GEN_ALT_LEN_MAX 255u
#define GEN_L_MAX 256u
#define GEN_NALT_MAX (1u << 22)
#define GEN_POOL_MAX (1u << 28)
#define GEN_HEADER_BYTES 16u

/* what gen_blob_check reads out of a blob that it accepts */
typedef struct {
  uint32_t npos, nalt, pool_bytes;
  uint32_t L;                     /* the longest candidate */
  uint64_t T;                     /* candidates */
  uint32_t count[GEN_POS_MAX], first[GEN_POS_MAX];
  uint32_t alt_at, pool_at;       /* byte offsets of alt[] and of the pool in the blob */
} gen_info;

static uint32_t gen_rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static void gen_wr32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24); }
static size_t gen_blob_bytes(uint32_t npos, uint32_t nalt, uint32_t pool_bytes) { return GEN_HEADER_BYTES + 8u * (size_t)npos + 8u * (size_t)nalt + pool_bytes; }

/* the validator: NULL and *gi filled, or why the blob is refused */
static const char *gen_blob_check(const uint8_t *blob, size_t bytes, gen_info *gi) {
  memset(gi, 0, sizeof *gi);
  if (!blob || bytes < GEN_HEADER_BYTES) return "the template is shorter than its header";
  if (memcmp(blob, "GEN\0", 4) != 0) return "the template does not start with the magic \"GEN\\0\"";
  if (blob[5] | blob[6] | blob[7]) return "the template's three zero bytes are not zero";
  const uint32_t npos = blob[4], nalt = gen_rd32(blob + 8), pool_bytes = gen_rd32(blob + 12);
  if (npos < 1 || npos > GEN_POS_MAX) return "a template has 1 ... 16 positions";
  if (nalt < 1 || nalt > GEN_NALT_MAX) return "a template has 1 ... 2^22 alternatives in all";
  if (pool_bytes > GEN_POOL_MAX) return "a template has at most 2^28 bytes of alternatives";
  if (bytes != gen_blob_bytes(npos, nalt, pool_bytes)) return "the template's length is not 16 + 8 npos + 8 nalt + pool_bytes";
  gi->npos = npos, gi->nalt = nalt, gi->pool_bytes = pool_bytes;
  gi->alt_at = GEN_HEADER_BYTES + 8u * npos, gi->pool_at = gi->alt_at + 8u * nalt;
  uint64_t next = 0, T = 1;
  uint32_t L = 0;
  for (uint32_t p = 0; p < npos; ++p) {
    const uint32_t count = gen_rd32(blob + GEN_HEADER_BYTES + 8u * p), first = gen_rd32(blob + GEN_HEADER_BYTES + 8u * p + 4);
    if (count < 1) return "a position of the template has no alternative";
    if (first != next || next + count > nalt) return "the positions' counts and first alternatives do not add up to nalt";
    next += count;
    uint32_t longest = 0;
    for (uint32_t a = first; a < first + count; ++a) {
      const uint32_t off = gen_rd32(blob + gi->alt_at + 8u * (size_t)a), len = gen_rd32(blob + gi->alt_at + 8u * (size_t)a + 4);
      if (len > GEN_ALT_LEN_MAX) return "an alternative of the template is longer than 255 bytes";
      if ((uint64_t)off + len > pool_bytes) return "an alternative of the template lies outside the pool";
      if (len > longest) longest = len;
    }
    L += longest;
    if (__builtin_mul_overflow(T, (uint64_t)count, &T)) return "the template has 2^64 candidates or more";
    gi->count[p] = count, gi->first[p] = first;
  }
  if (next != nalt) return "the positions' counts and first alternatives do not add up to nalt";
  if (L > GEN_L_MAX) return "the template's candidates are longer than 256 bytes";
  gi->L = L, gi->T = T;
  return NULL;
}

/* candidate i of an accepted blob, by plain division and remainder (the device steps an odometer: csrc/gen.h): its bytes to out[256],
   -> its length */
static uint32_t gen_candidate_host(const uint8_t *blob, const gen_info *gi, uint64_t i, uint8_t *out) {
  uint32_t digit[GEN_POS_MAX];
  for (uint32_t p = gi->npos; p-- > 0;) digit[p] = (uint32_t)(i % gi->count[p]), i /= gi->count[p];
  uint32_t len = 0;
  for (uint32_t p = 0; p < gi->npos; ++p) {
    const uint8_t *e = blob + gi->alt_at + 8u * (size_t)(gi->first[p] + digit[p]);
    const uint32_t off = gen_rd32(e), l = gen_rd32(e + 4);
    memcpy(out + len, blob + gi->pool_at + off, l);
    len += l;
  }
  return len;
}

/* ---- building a blob: positions in order, each position's alternatives in order */
typedef struct {
  uint32_t npos, count[GEN_POS_MAX];
  uint32_t nalt, alt_cap;
  uint32_t *off, *len;
  uint8_t *pool;
  size_t pool_bytes, pool_cap;
  int failed; /* out of memory, or past a limit of the format: the builder's caller reports it once, at the end */
} gen_build;

static void gen_build_free(gen_build *b) {
  free(b->off), free(b->len), free(b->pool);
  memset(b, 0, sizeof *b);
}
/* a new position (none yet, or after the alternatives of the one before): false past 16 */
static int gen_build_pos(gen_build *b) {
  if (b->npos >= GEN_POS_MAX) return 0;
  b->count[b->npos++] = 0;
  return 1;
}
/* one more alternative of the position in hand */
static void gen_build_alt(gen_build *b, const uint8_t *bytes, size_t n) {
  if (b->failed || !b->npos || n > GEN_ALT_LEN_MAX || b->nalt >= GEN_NALT_MAX || b->pool_bytes + n > GEN_POOL_MAX) { b->failed = 1; return; }
  if (b->nalt == b->alt_cap) {
    const uint32_t cap = b->alt_cap ? b->alt_cap * 2 : 64;
    uint32_t *o = (uint32_t *)realloc(b->off, (size_t)cap * 4), *l = o ? (uint32_t *)realloc(b->len, (size_t)cap * 4) : NULL;
    if (o) b->off = o;
    if (l) b->len = l;
    if (!o || !l) { b->failed = 1; return; }
    b->alt_cap = cap;
  }
  if (b->pool_bytes + n > b->pool_cap) {
    size_t cap = b->pool_cap ? b->pool_cap * 2 : 1024;
    while (cap < b->pool_bytes + n) cap *= 2;
    uint8_t *q = (uint8_t *)realloc(b->pool, cap);
    if (!q) { b->failed = 1; return; }
    b->pool = q, b->pool_cap = cap;
  }
  if (n) memcpy(b->pool + b->pool_bytes, bytes, n);
  b->off[b->nalt] = (uint32_t)b->pool_bytes, b->len[b->nalt] = (uint32_t)n;
  b->pool_bytes += n, b->nalt++, b->count[b->npos - 1]++;
}
/* the blob (malloc'ed, *bytes long), or NULL when the builder failed */
static uint8_t *gen_build_blob(const gen_build *b, size_t *bytes) {
  if (b->failed || !b->npos) return NULL;
  *bytes = gen_blob_bytes(b->npos, b->nalt, (uint32_t)b->pool_bytes);
  uint8_t *blob = (uint8_t *)calloc(*bytes, 1);
  if (!blob) return NULL;
  memcpy(blob, "GEN", 4), blob[4] = (uint8_t)b->npos;
  gen_wr32(blob + 8, b->nalt), gen_wr32(blob + 12, (uint32_t)b->pool_bytes);
  uint8_t *q = blob + GEN_HEADER_BYTES;
  uint32_t first = 0;
  for (uint32_t p = 0; p < b->npos; ++p, q += 8) gen_wr32(q, b->count[p]), gen_wr32(q + 4, first), first += b->count[p];
  for (uint32_t a = 0; a < b->nalt; ++a, q += 8) gen_wr32(q, b->off[a]), gen_wr32(q + 4, b->len[a]);
  if (b->pool_bytes) memcpy(q, b->pool, b->pool_bytes);
  return blob;
}

/* ---- the command line's mask and sets */
#define GEN_SPECIALS " !\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"
/* the bytes of class ?c, NULL if there is none */
static const char *gen_class(char c) {
  switch (c) {
  case 'l': return "abcdefghijklmnopqrstuvwxyz";
  case 'u': return "ABCDEFGHIJKLMNOPQRSTUVWXYZ";
  case 'd': return "0123456789";
  case 'h': return "0123456789abcdef";
  case 's': return GEN_SPECIALS;
  case 'a': return "abcdefghijklmnopqrstuvwxyz" "ABCDEFGHIJKLMNOPQRSTUVWXYZ" "0123456789" GEN_SPECIALS;
  default: return NULL;
  }
}
/* the lines of a word list as alternatives of the position in hand: cut at '\n', one '\r' before it dropped, empty lines skipped;
   a line is cut into pieces of 255 bytes no further - a longer one is refused (-1).  -> words taken */
static long gen_words(gen_build *b, const uint8_t *text, size_t len) {
  long n = 0;
  for (size_t at = 0; at < len;) {
    const uint8_t *nl = (const uint8_t *)memchr(text + at, '\n', len - at);
    const size_t stop = nl ? (size_t)(nl - text) : len;
    size_t l = stop - at;
    if (l && text[at + l - 1] == '\r') l--;
    if (l > GEN_ALT_LEN_MAX) return -1;
    if (l) gen_build_alt(b, text + at, l), ++n;
    at = stop + 1;
  }
  return n;
}
/* -1 ... -4 <spec> into `set` (a builder with one position): 0, or why[] says what is wrong */
static int gen_parse_set(const char *spec, char name, gen_build *set, char *why, size_t why_len) {
  memset(set, 0, sizeof *set);
  gen_build_pos(set);
  if (spec[0] == '@') {
    FILE *f = fopen(spec + 1, "rb");
    if (!f) return snprintf(why, why_len, "-%c: cannot read the word list '%s'", name, spec + 1), -1;
    size_t cap = 1 << 16, have = 0, got;
    uint8_t *text = (uint8_t *)malloc(cap);
    while (text && (got = fread(text + have, 1, cap - have, f)) > 0) {
      have += got;
      if (have == cap) {
        uint8_t *q = (uint8_t *)realloc(text, cap *= 2);
        if (!q) free(text);
        text = q;
      }
    }
    fclose(f);
    if (!text) return snprintf(why, why_len, "-%c: out of memory for the word list '%s'", name, spec + 1), -1;
    const long n = gen_words(set, text, have);
    free(text);
    if (n < 0) return snprintf(why, why_len, "-%c: a word of '%s' is longer than 255 bytes", name, spec + 1), -1;
    if (n == 0) return snprintf(why, why_len, "-%c: the word list '%s' holds no word", name, spec + 1), -1;
    if (set->failed) return snprintf(why, why_len, "-%c: the word list '%s' has more than 2^22 words or 2^28 bytes", name, spec + 1), -1;
    return 0;
  }
  uint8_t seen[256] = {0};
  for (const char *s = spec; *s; ++s) {
    const char *cls = NULL;
    char one[2] = {*s, 0};
    if (*s == '?') {
      ++s;
      if (*s == '?') one[0] = '?';
      else if (!*s || !(cls = gen_class(*s))) return snprintf(why, why_len, "-%c: unknown class ?%c (one of ?l ?u ?d ?h ?s ?a, or ?? for a '?')", name, *s ? *s : ' '), -1;
    }
    for (const char *c = cls ? cls : one; *c; ++c) {
      if (seen[(uint8_t)*c]) return snprintf(why, why_len, "-%c: the byte '%c' is in the set twice", name, *c), -1;
      seen[(uint8_t)*c] = 1;
      gen_build_alt(set, (const uint8_t *)c, 1);
    }
    if (!*s) break;
  }
  if (!set->nalt) return snprintf(why, why_len, "-%c: the set is empty", name), -1;
  return 0;
}
/* the mask into `out`; sets[k] is the set of ?<k + 1>, or NULL.  0, or why[] says what is wrong */
static int gen_parse_mask(const char *mask, const gen_build *const sets[4], gen_build *out, char *why, size_t why_len) {
  memset(out, 0, sizeof *out);
  uint8_t run[GEN_ALT_LEN_MAX];
  size_t nrun = 0;
  const char *const too_many = "invalid -mask: more than 16 positions";
#define GEN_FLUSH_RUN()                                                                  \
  do {                                                                                   \
    if (nrun) {                                                                          \
      if (!gen_build_pos(out)) return snprintf(why, why_len, "%s", too_many), -1;        \
      gen_build_alt(out, run, nrun), nrun = 0;                                           \
    }                                                                                    \
  } while (0)
  for (const char *s = mask; *s; ++s) {
    if (*s != '?' || s[1] == '?') { /* a literal byte; a run longer than an alternative may be goes on as another position */
      if (*s == '?') ++s;
      if (nrun == GEN_ALT_LEN_MAX) GEN_FLUSH_RUN();
      run[nrun++] = (uint8_t)*s;
      continue;
    }
    ++s;
    GEN_FLUSH_RUN();
    if (*s >= '1' && *s <= '4') {
      const gen_build *set = sets[*s - '1'];
      if (!set) return snprintf(why, why_len, "invalid -mask: ?%c needs -%c <set>", *s, *s), -1;
      if (!gen_build_pos(out)) return snprintf(why, why_len, "%s", too_many), -1;
      for (uint32_t a = 0; a < set->nalt; ++a) gen_build_alt(out, set->pool + set->off[a], set->len[a]);
      continue;
    }
    const char *cls = *s ? gen_class(*s) : NULL;
    if (!cls) return snprintf(why, why_len, "invalid -mask: unknown class ?%c (one of ?l ?u ?d ?h ?s ?a ?1 ?2 ?3 ?4, or ?? for a '?')", *s ? *s : ' '), -1;
    if (!gen_build_pos(out)) return snprintf(why, why_len, "%s", too_many), -1;
    for (const char *c = cls; *c; ++c) gen_build_alt(out, (const uint8_t *)c, 1);
    if (!*s) break;
  }
  GEN_FLUSH_RUN();
#undef GEN_FLUSH_RUN
  if (!out->npos) return snprintf(why, why_len, "invalid -mask: the template is empty"), -1;
  if (out->failed) return snprintf(why, why_len, "invalid -mask: more than 2^22 alternatives or 2^28 bytes of them, or out of memory"), -1;
  return 0;
}
#endif
