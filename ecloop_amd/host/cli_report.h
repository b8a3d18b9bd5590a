/* cli_report.h - report_t (found sink, status line, pause state) and run_t (one run of a search command).
   Part of the one translation unit ecloop_hip_cli.c (included there, in this order). */
/* ------------------------------------------------------------------------------------------- found sink + status line */
/* One object for everything the program reports while it runs: found keys (stdout unless -q, the -o file), the two
   counters behind the status line, the clock with the paused time taken out.  Formats are the reference's
   (ctx_write_found main.c:182-203, ctx_print_status main.c:134-144, ctx_update main.c:158-172), byte for byte; the device
   threads and the key listener share it through its mutex. */
typedef struct {
  pthread_mutex_t mu;
  FILE *file;      /* -o (appended to), or NULL */
  bool quiet;      /* -q: nothing on stdout */
  u64 found, checked;
  bool prefix;     /* -p: the status line shows `edge` as well */
  u64 edge;        /* -p: records dropped because their address text matched no pattern (a range's end values) */
  bool brain;      /* brain: the status line shows the candidate index reached and the template's count as well (a run resumes with -r) */
  u64 brain_at, brain_T;
  u64 t_start, t_progress, t_shown; /* ms: clock start, last progress report, last status print */
  u64 paused_ms, paused_since;
  volatile bool paused; /* read by the device threads without the mutex, like the reference's flag (main.c:153) */
  bool closed;
} report_t;

static void hex_of_words(char *dst, const u32 *w, int n) { /* 8 digits per word, most significant word first as given */
  for (int i = 0; i < n; ++i) sprintf(dst + 8 * i, "%08x", w[i]);
}
static void hex_of_scalar(char dst[65], const sc *k) {
  for (int i = 0; i < 4; ++i) sprintf(dst + 16 * i, "%016llx", (unsigned long long)k->w[3 - i]);
}
static void report_init(report_t *r, const char *outfile, bool quiet) {
  memset(r, 0, sizeof *r);
  pthread_mutex_init(&r->mu, NULL);
  r->quiet = quiet;
  if (outfile) r->file = fopen(outfile, "a");
  r->t_start = r->t_progress = ms_now();
  r->t_shown = r->t_start - 5000;
}
static void report_restart_clock(report_t *r) { r->t_start = ms_now(); } /* the commands start their clock after bring-up */
/* "<secs>s ~ <rate> Mkeys/s ~ <found> / <checked>" + the key hint; '\r' while running, '\n' once closed */
static void status_show_locked(report_t *r) {
  int64_t run_ms = (int64_t)(r->t_progress - r->t_start) - (int64_t)r->paused_ms;
  double secs = (run_ms < 1 ? 1 : run_ms) / 1000.0;
  const char *hint = r->closed ? "" : r->paused ? " ('r' \xe2\x80\x93 resume)" : " ('p' \xe2\x80\x93 pause)";
  erase_status_line();
  char edge[64] = "";
  if (r->prefix) snprintf(edge, sizeof edge, " ~ edge: %llu", (unsigned long long)r->edge);
  if (r->brain) snprintf(edge, sizeof edge, " ~ index: %llx / %llx", (unsigned long long)r->brain_at, (unsigned long long)r->brain_T);
  fprintf(stderr, "%.2fs ~ %.2f Mkeys/s ~ %'llu / %'llu%s%s%c", secs, r->checked / secs / 1000000, (unsigned long long)r->found,
          (unsigned long long)r->checked, edge, hint, r->closed ? '\n' : '\r');
  fflush(stderr);
}
/* one found key: "addr33: <hash160> <- <key>" on stdout, "addr33\t<hash160>\t<key>" in the file; counts it.  type: the address type of
   ecl_found.compressed (1 addr33, 0 addr65, 2 p2sh, 3 eth, 4 p2tr, 5 pub - the last four have no reference counterpart, their labels are this
   program's).  A p2tr hit is printed with all 32 bytes of its output key (h: the eight words of ecl_hip_verify_tr), the others with the 20
   bytes of the record */
static void report_line(report_t *r, const char *label, const char *hh, const sc *key) {
  char kk[65];
  hex_of_scalar(kk, key);
  const struct { FILE *to; const char *fmt; } dest[2] = {{r->quiet ? NULL : stdout, "%s: %s <- %s\n"}, {r->file, "%s\t%s\t%s\n"}};
  pthread_mutex_lock(&r->mu);
  for (int d = 0; d < 2; ++d) {
    if (!dest[d].to) continue;
    if (dest[d].to == stdout) erase_status_line();
    fprintf(dest[d].to, dest[d].fmt, label, hh, kk);
    fflush(dest[d].to);
  }
  r->found++;
  status_show_locked(r);
  pthread_mutex_unlock(&r->mu);
}
/* A pub hit (type 5, -a x) is printed as the compressed public key of the key that was walked, re-derived: h = the eight words of x and,
   as a ninth, the parity of y (verify_hits) - "pub: <02 / 03><64 hex digits> <- <key>" */
static void report_hit(report_t *r, u8 type, const u32 *h, const sc *key) {
  char hh[67];
  if (type == 5) snprintf(hh, 3, "%02x", 2u | (h[8] & 1u)), hex_of_words(hh + 2, h, 8);
  else hex_of_words(hh, h, type == 4 ? 8 : 5);
  report_line(r, type == 5 ? "pub" : type == 4 ? "p2tr" : type == 3 ? "eth" : type == 2 ? "p2sh" : type ? "addr33" : "addr65", hh, key);
}
/* `units` more keys checked (status units: the reference counts job_size per job, x6 with -endo, main.c:431); the line
   is redrawn at most every 100 ms; a paused run parks the caller here, between two device calls */
static void report_progress(report_t *r, u64 units) {
  u64 now = ms_now();
  pthread_mutex_lock(&r->mu);
  r->checked += units, r->t_progress = now;
  if (now - r->t_shown >= 100) r->t_shown = now, status_show_locked(r);
  pthread_mutex_unlock(&r->mu);
  while (r->paused) usleep(100000);
}
static void report_pause(report_t *r, bool on) { /* 'p' / 'r' (main.c:874-888): paused time does not count */
  pthread_mutex_lock(&r->mu);
  if (on != r->paused) {
    u64 now = ms_now();
    if (on) r->paused_since = now;
    else r->paused_ms += now - r->paused_since;
    r->paused = on;
    status_show_locked(r);
  }
  pthread_mutex_unlock(&r->mu);
}
static void report_close(report_t *r) { /* ctx_finish, main.c:174-180 */
  pthread_mutex_lock(&r->mu);
  r->closed = true, r->t_progress = ms_now();
  status_show_locked(r);
  if (r->file) fclose(r->file), r->file = NULL;
  pthread_mutex_unlock(&r->mu);
}

/* ------------------------------------------------------------------------------------------- one run of a search command */
enum { CMD_NIL, CMD_ADD, CMD_MUL, CMD_RND };
typedef struct run_t {
  int cmd;
  opts_t opt;
  filter_t flt;
  report_t rep;
  int ngpus; /* device contexts (threads); `mul` opens two per GPU */
  ecl_hip *dev[MAX_GPUS];
  bool a33, a65, p2sh, eth, tr, pub, endo, colour, bin, parse_only, seeded;
  int kdf; /* mul -raw: KDF_* of -kdf (keccak_host.h), 0 = SHA-256 */
  sc range_s, range_e, stride_k;
  u32 ord_offs, ord_size;
  pfx_plan *pfx; /* -p: the plan of the patterns (cli_prefix.h), NULL otherwise */
  msk_plan *msk; /* -p with a 0x pattern that has ? or *: the mask plan; pfx then holds the patterns alone, no ranges */
  bool split;    /* -p with -k: the walk starts from the requester's public key (cli_splitkey.h); the keys reported are partial keys */
  u64 origin[8]; /* ... its x and y, the last eight of the twelve limbs of every add_range call */
  char split_hex[67];
} run_t;

/* A failed library call ends the run.  Device threads can fail at the same time (`mul`'s two contexts of a GPU): the first one reports and
   ends the process, the others wait here - two threads in exit() at once, or the HIP runtime's teardown under another thread's calls,
   crash the process instead of ending it with status 1.  _exit runs no atexit handlers: the streams and the terminal (cli_keys.h) are
   seen to here. */
static void keys_restore(void);
static void die_ecl(run_t *run, int g, int rc, const char *what) {
  static pthread_mutex_t once = PTHREAD_MUTEX_INITIALIZER;
  pthread_mutex_lock(&once);
  fprintf(stderr, "\n[!] %s: %s (%s)\n", what, ecl_hip_strerror(rc), run->dev[g] ? ecl_hip_last_error(run->dev[g]) : "");
  fflush(NULL);
  keys_restore();
  _exit(1);
}
/* The hit records of a device call, and the caller's half of the overflow protocol (include/ecloop_hip.h).  A search call that reports more
   hits than its buffer holds (ECL_E_OVERFLOW: a dense filter) has kept up to max(cap, 2^20) of them on the device, and they are read from
   there.  A call with more hits than the device keeps - 2^19 + 1 keys of `-a cu` through an all-ones filter are enough - has to be made
   again with a buffer that fits.  Every command that searches goes through here. */
typedef struct { ecl_found *rec; u32 cap; } hits_t;
static void hits_room(hits_t *b, u32 cap) { /* room for cap records, what b holds stays; a failed allocation ends the program */
  if (cap <= b->cap) return;
  b->rec = realloc(b->rec, sizeof(ecl_found) * cap), b->cap = cap;
  if (!b->rec) { fprintf(stderr, "out of memory for %u hit records\n", cap); exit(1); }
}
/* behind a search call that returned *rc and reported cnt hits into b.  ECL_E_OVERFLOW: b grows to cnt and records [old cap, cnt) are
   fetched.  -> true: the device kept fewer than the call produced - b now holds room for cnt, the same call made again fits.
   -> false: *rc is the call's result (ECL_OK: b holds all cnt records). */
static bool hits_need_repeat(ecl_hip *h, int *rc, hits_t *b, u32 cnt) {
  if (*rc != ECL_E_OVERFLOW) return false;
  const u32 had = b->cap;
  u32 got = 0;
  hits_room(b, cnt);
  *rc = ecl_hip_fetch_found(h, had, b->rec + had, cnt - had, &got);
  return *rc == ECL_OK && got != cnt - had;
}
/* pk_verify_hash (main.c:248-263) for all hits of one device call at once: both hash160 values of every reported key are
   derived again on the device by the window-table sum (ecl_hip_verify: not the walk kernel; own inversion per key) and
   compared with what the walk reported; a p2sh hit is compared with the script hash of that addr33 hash (ecl_hip_p2sh_hash);
   an eth hit with the address ecl_hip_verify_eth derives from the key (an eth run has no other hits); a p2tr hit with the first 20 bytes
   of the output key ecl_hip_verify_tr derives (a Taproot run has no other hits), whose 32 bytes go to `full` for the found line;
   a pub hit with the first 20 bytes of the x of the key's point from ecl_hip_diag_mulg, whose 32 bytes and the parity of y go to `full`;
   a mismatch is fatal, with the reference's diagnostics */
static void verify_fail(const sc *key, const ecl_found *hit, const u32 *want) {
  char kk[65], lh[41], rh[41];
  hex_of_scalar(kk, key), hex_of_words(lh, hit->h160, 5), hex_of_words(rh, want, 5);
  fprintf(stderr, "[!] error: hash mismatch (compressed: %d endo: %d)\npk: %s\nlh: %s\nrh: %s\n", hit->compressed, hit->endo, kk, lh, rh);
  exit(1);
}
#define FULL_WORDS 9 /* a whole key for the found line: eight words (p2tr: the output key; pub: x) and the parity of y (pub) */
static void verify_hits(run_t *run, int g, const sc *keys, const ecl_found *hits, u32 n, u32 (*full)[FULL_WORDS]) {
  if (!n) return;
  if (run->split) { /* -p with -k: the point of a hit is Q + k G; its image `endo` is O' + k' G, k' = keys[i] (calc_priv's) and O' the same image
                       of Q (splitkey.h) - twelve limbs per entry, re-derived by the window-table sum + O' (ecl_hip_verify on such a context) */
    u64 (*ent)[12] = malloc((size_t)n * sizeof *ent);
    u32 (*h33)[5] = malloc((size_t)n * 20), (*h65)[5] = malloc((size_t)n * 20);
    u8 *fin = malloc(n);
    for (u32 i = 0; i < n; ++i) {
      memcpy(ent[i], keys[i].w, 32), memcpy(ent[i] + 4, run->origin, 64);
      sk_image_origin(ent[i] + 4, ent[i] + 8, hits[i].endo);
    }
    int rc = run->eth ? ecl_hip_verify_eth(run->dev[g], (const uint64_t(*)[4])ent, n, h33, fin)
                      : ecl_hip_verify(run->dev[g], (const uint64_t(*)[4])ent, n, h33, h65, fin);
    if (rc != ECL_OK) die_ecl(run, g, rc, "verify");
    for (u32 i = 0; i < n; ++i) {
      const u32 *want = run->eth || hits[i].compressed ? h33[i] : h65[i];
      if (hits[i].compressed != (run->eth ? 3 : hits[i].compressed ? 1 : 0) || !fin[i] || memcmp(want, hits[i].h160, 20)) verify_fail(&keys[i], &hits[i], want);
    }
    free(ent), free(h33), free(h65), free(fin);
    return;
  }
  if (run->pub) { /* the key's point by the double-and-add kernel (ecl_hip_diag_mulg: neither the walk nor the window sum), x and y */
    u64 (*x)[4] = malloc((size_t)n * 32), (*y)[4] = malloc((size_t)n * 32);
    u8 *fin = malloc(n);
    int rc = ecl_hip_diag_mulg(run->dev[g], (const uint64_t(*)[4])keys, x, y, fin, n);
    if (rc != ECL_OK) die_ecl(run, g, rc, "verify");
    for (u32 i = 0; i < n; ++i) {
      for (int j = 0; j < 8; ++j) full[i][j] = (u32)(x[i][(7 - j) / 2] >> (32 * ((7 - j) & 1)));
      full[i][8] = (u32)(y[i][0] & 1);
      if (hits[i].compressed != 5 || !fin[i] || memcmp(full[i], hits[i].h160, 20)) verify_fail(&keys[i], &hits[i], full[i]);
    }
    free(x), free(y), free(fin);
    return;
  }
  if (run->tr) {
    u8 *fin = malloc(n);
    u32 (*qx)[8] = malloc((size_t)n * 32);
    int rc = ecl_hip_verify_tr(run->dev[g], (const uint64_t(*)[4])keys, n, qx, fin);
    if (rc != ECL_OK) die_ecl(run, g, rc, "verify");
    for (u32 i = 0; i < n; ++i) {
      memcpy(full[i], qx[i], 32), full[i][8] = 0;
      if (hits[i].compressed != 4 || !fin[i] || memcmp(qx[i], hits[i].h160, 20)) verify_fail(&keys[i], &hits[i], qx[i]);
    }
    free(fin), free(qx);
    return;
  }
  if (run->eth) {
    u32 (*addr)[5] = malloc((size_t)n * 20);
    u8 *fin = malloc(n);
    int rc = ecl_hip_verify_eth(run->dev[g], (const uint64_t(*)[4])keys, n, addr, fin);
    if (rc != ECL_OK) die_ecl(run, g, rc, "verify");
    for (u32 i = 0; i < n; ++i)
      if (hits[i].compressed != 3 || !fin[i] || memcmp(addr[i], hits[i].h160, 20)) verify_fail(&keys[i], &hits[i], addr[i]);
    free(addr), free(fin);
    return;
  }
  u32 (*h33)[5] = malloc((size_t)n * 20), (*h65)[5] = malloc((size_t)n * 20), (*hsh)[5] = NULL;
  u8 *finite = malloc(n);
  int rc = ecl_hip_verify(run->dev[g], (const uint64_t(*)[4])keys, n, h33, h65, finite);
  if (rc != ECL_OK) die_ecl(run, g, rc, "verify");
  if (run->p2sh) {
    hsh = malloc((size_t)n * 20);
    rc = ecl_hip_p2sh_hash(run->dev[g], (const uint32_t(*)[5])h33, hsh, n);
    if (rc != ECL_OK) die_ecl(run, g, rc, "verify");
  }
  for (u32 i = 0; i < n; ++i) {
    const u32 *want = hits[i].compressed == 2 && hsh ? hsh[i] : hits[i].compressed ? h33[i] : h65[i];
    if (finite[i] && !memcmp(want, hits[i].h160, 20)) continue;
    verify_fail(&keys[i], &hits[i], want);
  }
  free(h33), free(h65), free(hsh), free(finite);
}
