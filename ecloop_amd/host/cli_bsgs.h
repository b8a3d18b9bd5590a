/* cli_bsgs.h - the `bsgs` command: baby-step giant-step search for the private key of a KNOWN public key in a range (no reference
   counterpart).  Part of the one translation unit ecloop_hip_cli.c (included there, in this order).
   The method and its arithmetic are host/bsgs_plan.h's; here: the command line, the three device contexts and the resolution of records.
     ecloop-hip bsgs -k <pubkey | file of pubkeys> -r a:b [-b beta] [-m words] [-o file] [-q]
   The baby filter is built once on an ECL_PUB | ECL_INSERT context, read back into page-locked host memory and uploaded into the
   ECL_PUB | ECL_ORIGIN context that walks the giant steps of every target; a record names a giant step, whose window of s keys an ordinary
   ECL_PUB context rescans (device list: the one entry of the target's x); a key is accepted only if all 32 bytes of x and the parity of y
   of its re-derived point (ecl_hip_diag_mulg) are the target's.  A window that yields nothing was a bloom false positive: counted, and
   the walk goes on.  One GPU. */
#include "bsgs_plan.h"

typedef struct { u64 x[4], y[4]; char hex[67]; } bsgs_target;

static void bsgs_die(ecl_hip *h, int rc, const char *what) {
  fprintf(stderr, "\n[!] %s: %s (%s)\n", what, ecl_hip_strerror(rc), h ? ecl_hip_last_error(h) : "");
  fflush(NULL);
  _exit(1);
}
/* 64 hex digits -> four little-endian limbs */
static bool bsgs_limbs_from_hex(const char *s, u64 v[4]) {
  u32 w[8];
  if (!words8_from_hex(s, w)) return false;
  for (int i = 0; i < 4; ++i) v[i] = (u64)w[6 - 2 * i] << 32 | w[7 - 2 * i];
  return true;
}
/* one public key: 66 digits (02 / 03: y is lifted) or 130 digits (04: checked on the curve); a bare x names two keys and is refused */
static bool bsgs_parse_key(const char *s, size_t n, bsgs_target *t) {
  while (n && isspace((unsigned char)s[n - 1])) --n;
  if (n == 66 && s[0] == '0' && (s[1] == '2' || s[1] == '3')) {
    if (!bsgs_limbs_from_hex(s + 2, t->x) || !bsgs_lift_x(t->y, t->x, s[1] == '3')) return false;
  } else if (n == 130 && s[0] == '0' && s[1] == '4') {
    if (!bsgs_limbs_from_hex(s + 2, t->x) || !bsgs_limbs_from_hex(s + 66, t->y) || !bsgs_on_curve(t->x, t->y)) return false;
  } else return false;
  snprintf(t->hex, sizeof t->hex, "%02x%016llx%016llx%016llx%016llx", 2u | (unsigned)(t->y[0] & 1), (unsigned long long)t->x[3],
           (unsigned long long)t->x[2], (unsigned long long)t->x[1], (unsigned long long)t->x[0]);
  return true;
}
static void bsgs_bad_key(const char *s, size_t n) {
  while (n && isspace((unsigned char)s[n - 1])) --n;
  fprintf(stderr, "invalid public key '%.*s': 66 hex digits (02.. / 03..) or 130 (04.., on the curve)%s\n", (int)(n > 140 ? 140 : n), s,
          n == 64 ? "; a bare x names two keys" : "");
  exit(1);
}
/* -k: a key, or a file of keys (one per line; empty lines skipped) */
static bsgs_target *bsgs_targets(const char *arg, size_t *count) {
  bsgs_target *t = NULL;
  *count = 0;
  FILE *f = fopen(arg, "r");
  if (!f) {
    t = malloc(sizeof *t);
    if (!bsgs_parse_key(arg, strlen(arg), t)) bsgs_bad_key(arg, strlen(arg));
    *count = 1;
    return t;
  }
  size_t len = 0, cap = 0;
  char *text = slurp(f, &len);
  fclose(f);
  for (size_t at = 0; at < len;) {
    const char *eol = memchr(text + at, '\n', len - at);
    size_t n = eol ? (size_t)(eol - (text + at)) : len - at, m = n;
    while (m && isspace((unsigned char)text[at + m - 1])) --m;
    if (m) {
      if (*count == cap) t = realloc(t, (cap = cap ? 2 * cap : 16) * sizeof *t);
      if (!bsgs_parse_key(text + at, m, &t[*count])) bsgs_bad_key(text + at, m);
      ++*count;
    }
    at += n + 1;
  }
  free(text);
  if (!*count) { fprintf(stderr, "no public keys in '%s'\n", arg); exit(1); }
  return t;
}
/* -r a:b, both ends in hex, both inclusive */
static void bsgs_range(const char *raw, bsgs_int *a, bsgs_int *b) {
  const char *sep = raw ? strchr(raw, ':') : NULL;
  if (!sep || sep == raw || !sep[1] || strlen(sep + 1) > 64 || sep - raw > 64 || strspn(raw, "0123456789abcdefABCDEF:") != strlen(raw)) {
    fprintf(stderr, "invalid search range, use format: -r 8000:ffff\n");
    exit(1);
  }
  char head[65] = {0};
  memcpy(head, raw, (size_t)(sep - raw));
  const sc lo = sc_from_hex(head), hi = sc_from_hex(sep + 1);
  memcpy(a->w, lo.w, 32), memcpy(b->w, hi.w, 32);
}
/* a found key in the formats of the found sink (cli_report.h): "pub: <compressed key> <- <key>" on stdout unless -q, tab-separated in the -o file */
static void bsgs_found(FILE *file, bool quiet, const char *hex, const bsgs_int *key) {
  char kk[65];
  sc k;
  memcpy(k.w, key->w, 32);
  hex_of_scalar(kk, &k);
  if (!quiet) erase_status_line(), printf("pub: %s <- %s\n", hex, kk), fflush(stdout);
  if (file) fprintf(file, "pub\t%s\t%s\n", hex, kk), fflush(file);
}
static int bsgs_order(const void *p, const void *q) {
  const u64 a = ((const ecl_found *)p)->key_offset, b = ((const ecl_found *)q)->key_offset;
  return a < b ? -1 : a > b;
}
static void bsgs_status(bool quiet, const bsgs_int *done, const bsgs_int *steps, u64 fp, bool last) {
  if (quiet) return;
  erase_status_line();
  if (done->w[1] | done->w[2] | done->w[3] | steps->w[1] | steps->w[2] | steps->w[3])
    fprintf(stderr, "giant steps: 2^%u / 2^%u ~ false positives: %llu%c", bsgs_bits(done), bsgs_bits(steps), (unsigned long long)fp, last ? '\n' : '\r');
  else
    fprintf(stderr, "giant steps: %'llu / %'llu ~ false positives: %'llu%c", (unsigned long long)done->w[0], (unsigned long long)steps->w[0],
            (unsigned long long)fp, last ? '\n' : '\r');
  fflush(stderr);
}
#define BSGS_CAP 4096u
static int cmd_bsgs(const opts_t *o) {
  if (opt_number(o->gpus, 1) > 1) { fprintf(stderr, "bsgs runs on one GPU: -t %s is not supported (sharding the giant range is not implemented)\n", o->gpus); exit(1); }
  if (!o->pubkey) { fprintf(stderr, "bsgs: missing -k <pubkey | file of pubkeys>\n"); exit(1); }
  if (o->quiet && !o->outfile) { fprintf(stderr, "quiet mode chosen without output file\n"); exit(1); }
  bsgs_int a, b;
  bsgs_range(o->range, &a, &b);
  size_t ntargets = 0;
  bsgs_target *targets = bsgs_targets(o->pubkey, &ntargets);
  const bool auto_beta = !o->baby;
  unsigned beta = auto_beta ? bsgs_default_beta(&a, &b) : (unsigned)opt_number(o->baby, 0);
  if (!auto_beta && (beta > 32 || strspn(o->baby, "0123456789") != strlen(o->baby))) { fprintf(stderr, "invalid -b '%s': the number of baby steps is 2^b, b = 0 ... 32\n", o->baby); exit(1); }
  const u64 words_opt = opt_number(o->words, 0);
  if (o->words && (!words_opt || words_opt >= (1ull << 58))) { fprintf(stderr, "invalid -m '%s': the words of the baby filter\n", o->words); exit(1); }
  bsgs_plan plan;
  int prc = bsgs_plan_make(&plan, &a, &b, beta);
  if (prc == BSGS_E_ORDER) { fprintf(stderr, "invalid search range: bsgs needs 1 <= a <= b < n\n"); exit(1); }
  if (prc == BSGS_E_RANGE) { fprintf(stderr, "invalid search range: 2 (b + s) + 1 >= n (s = 2^%u) - a giant step could be the point at infinity\n", beta + 1); exit(1); }
  if (ecl_hip_device_count() <= 0) { fprintf(stderr, "no MI355X GPU visible (the search path has no CPU fallback)\n"); return 1; }
  FILE *outfile = o->outfile ? fopen(o->outfile, "a") : NULL;

  /* ---- the baby table: once, for every target */
  ecl_hip *ins = NULL, *giant = NULL, *scan = NULL;
  u64 nwords, *pin;
  int rc;
  const u64 t0 = ms_now();
  for (;;) {
    nwords = words_opt ? words_opt : bsgs_filter_words(&plan);
    pin = ecl_hip_alloc_host((size_t)nwords * 8);
    rc = pin ? ecl_hip_open(&ins, 0, ECL_PUB | ECL_INSERT, plan.baby_offs) : ECL_E_HIP;
    if (rc == ECL_OK) memset(pin, 0, (size_t)nwords * 8), rc = ecl_hip_set_bloom(ins, pin, nwords);
    if (rc == ECL_E_HIP && auto_beta && !words_opt && beta > BSGS_BETA_MIN) { /* the filter does not fit the memory that is free: fewer baby steps */
      if (ins) ecl_hip_close(ins), ins = NULL;
      ecl_hip_free_host(pin);
      bsgs_plan_make(&plan, &a, &b, --beta);
      continue;
    }
    if (rc != ECL_OK) bsgs_die(ins, rc, "baby filter");
    break;
  }
  u32 n = 0;
  rc = ecl_hip_add_range(ins, plan.baby_start.w, plan.baby_keys, NULL, 0, &n);
  if (rc == ECL_OK) rc = ecl_hip_get_bloom(ins, pin, nwords);
  if (rc != ECL_OK) bsgs_die(ins, rc, "baby steps");
  ecl_hip_close(ins);
  rc = ecl_hip_open(&giant, 0, ECL_PUB | ECL_ORIGIN, plan.giant_offs);
  if (rc == ECL_OK) rc = ecl_hip_set_bloom(giant, pin, nwords);
  if (rc != ECL_OK) bsgs_die(giant, rc, "giant context");
  ecl_hip_free_host(pin);
  if (!o->quiet) {
    printf("bsgs: %zu target%s ~ baby steps: 2^%u ~ giant steps: ", ntargets, ntargets == 1 ? "" : "s", beta);
    if (plan.steps.w[1] | plan.steps.w[2] | plan.steps.w[3]) printf("2^%u", bsgs_bits(&plan.steps));
    else printf("%'llu", (unsigned long long)plan.steps.w[0]);
    printf(" of %'llu keys | filter: %.0f MB\nsetup: %.2fs (baby table built and copied)\n----------------------------------------\n",
           (unsigned long long)plan.s, nwords * 8 / 1e6, (ms_now() - t0) / 1000.0);
    fflush(stdout);
  }

  hits_t hits = {NULL, 0}; /* kept, and what it grew to, across the calls and the targets */
  hits_room(&hits, BSGS_CAP);
  for (size_t t = 0; t < ntargets; ++t) {
    const bsgs_target *q = &targets[t];
    u64 start12[12], fp = 0;
    bsgs_origin(start12 + 4, start12 + 8, q->x, q->y);
    u32 entry[5];
    for (int j = 0; j < 5; ++j) entry[j] = (u32)(q->x[(7 - j) / 2] >> (32 * ((7 - j) & 1)));
    bool found = false, scan_ready = false;
    bsgs_int done = {{0, 0, 0, 0}}, call_start;
    u64 steps;
    while (!found && (steps = bsgs_giant_call(&plan, &done, &call_start)) != 0) {
      memcpy(start12, call_start.w, 32);
      rc = ecl_hip_add_range(giant, start12, steps, hits.rec, hits.cap, &n);
      if (hits_need_repeat(giant, &rc, &hits, n)) { /* (a thin filter; the walk is not made again) */
        fprintf(stderr, "\n[!] bsgs: more records in one call than the device keeps; use a larger filter (-m)\n");
        exit(1);
      }
      if (rc != ECL_OK) bsgs_die(giant, rc, "giant steps");
      ecl_found *recs = hits.rec;
      qsort(recs, n, sizeof *recs, bsgs_order);
      for (u32 r = 0; r < n && !found; ++r) {
        bsgs_int i = bsgs_u64(recs[r].key_offset), first;
        bsgs_add(&i, &i, &done);
        const u64 nk = bsgs_window(&plan, &i, &first);
        if (!scan) {
          rc = ecl_hip_open(&scan, 0, ECL_PUB, 0);
          if (rc == ECL_OK) rc = ecl_hip_set_lookahead(scan, 0);
          if (rc != ECL_OK) bsgs_die(scan, rc, "rescan context");
        }
        if (!scan_ready) { /* this target's x: a one-entry filter and the list that confirms it */
          u64 words[1024] = {0};
          filter_t one = {words, 1024, NULL, 0};
          bloom_set(&one, entry);
          rc = ecl_hip_set_bloom(scan, words, 1024);
          if (rc == ECL_OK) rc = ecl_hip_set_list(scan, (const uint32_t(*)[5])entry, 1);
          if (rc != ECL_OK) bsgs_die(scan, rc, "rescan filter");
          scan_ready = true;
        }
        ecl_found hit[64];
        u32 m = 0;
        rc = ecl_hip_add_range(scan, first.w, nk, hit, 64, &m);
        if (rc != ECL_OK && rc != ECL_E_OVERFLOW) bsgs_die(scan, rc, "rescan");
        for (u32 k = 0; k < (m < 64 ? m : 64) && !found; ++k) {
          bsgs_int key = bsgs_u64(hit[k].key_offset);
          bsgs_add(&key, &key, &first);
          u64 x[1][4], y[1][4];
          u8 fin = 0;
          rc = ecl_hip_diag_mulg(scan, (const uint64_t(*)[4])key.w, x, y, &fin, 1);
          if (rc != ECL_OK) bsgs_die(scan, rc, "verify");
          if (fin && !memcmp(x[0], q->x, 32) && (y[0][0] & 1) == (q->y[0] & 1)) {
            bsgs_found(outfile, o->quiet, q->hex, &key);
            found = true;
          }
        }
        if (!found) ++fp;
      }
      bsgs_int walked = bsgs_u64(steps);
      bsgs_add(&done, &done, &walked);
      bsgs_status(o->quiet, &done, &plan.steps, fp, false);
    }
    bsgs_status(o->quiet, &done, &plan.steps, fp, true);
    if (!found) fprintf(stderr, "%s not found\n", q->hex);
  }
  free(hits.rec), free(targets);
  if (outfile) fclose(outfile);
  ecl_hip_close(giant);
  if (scan) ecl_hip_close(scan);
  return 0;
}
