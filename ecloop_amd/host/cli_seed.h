/* cli_seed.h - `seed` (no reference counterpart): BIP39 phrases on stdin -> BIP32 keys on the device -> the address search of `mul`.
     ecloop-hip seed -f <list | .blf> [-a ...] [-path <p>]... [-n count] [-pass <text>] [-o file] [-q] < phrases.txt
   Stdin is read in chunks that end behind a newline, so its length has no bound.  Lines are cut as `mul -raw` cuts them and taken as
   given (no NFKD, no word list, no checksum test).  Up to 8 -path (m/44'/0'/0'/0/0, ' or h = hardened, at most 10 elements); -n (1 ... 1024) also searches the next count - 1 values of each path's last element.  Per batch of 2^20
   phrases ONE call hashes the phrases (reuse = 0 of ECL_KDF_BIP39, include/ecloop_hip.h); every further (path, index) is a reuse = 1 call that
   walks from the kept master nodes.  Every hit's key is recomputed here (bip39_host.h; the public keys of normal elements from
   ecl_hip_diag_mulg, the double-and-add kernel - neither the window sum of `mul` nor the table sum of the device's own derivation) and the hit is
   re-derived on the device from that key (verify_hits): a device derivation that disagrees ends the run with the hash mismatch error.
   Part of the one translation unit ecloop_hip_cli.c. */
#define SEED_PATHS_MAX 8
#define SEED_COUNT_MAX 1024u
#define SEED_BATCH (1u << 20)
#define SEED_RECORD_ROOM 160u /* the record's slot in front of a batch's text: 8 + 4 * 10 + 99 bytes at most */

typedef struct { u32 el[B32_DEPTH_MAX]; int depth; } seed_path;

static void seed_die(const char *fmt, const char *arg) {
  fprintf(stderr, fmt, arg);
  exit(1);
}
/* the key of `phrase` at `path`, on the host; dev: the context whose double-and-add kernel gives the public keys of normal elements
   (NULL: a path with such an element is the caller's mistake).  An invalid node gives the key 0. */
static sc seed_host_key(run_t *run, const u8 *phrase, size_t plen, const u8 *pass, size_t pass_len, const seed_path *path) {
  u8 seed[64], c[32];
  sc k;
  const sc zero = {{0, 0, 0, 0}};
  b39_seed(seed, phrase, plen, pass, pass_len);
  if (!b32_master(&k, c, seed)) return zero;
  for (int d = 0; d < path->depth; ++d) {
    u8 pub[33] = {0};
    if (!(path->el[d] & B32_HARDENED)) {
      u64 x[1][4], y[1][4];
      u8 fin = 0;
      const int rc = ecl_hip_diag_mulg(run->dev[0], (const uint64_t(*)[4])k.w, x, y, &fin, 1);
      if (rc != ECL_OK) die_ecl(run, 0, rc, "seed: public key of a path element");
      const sc xs = {{x[0][0], x[0][1], x[0][2], x[0][3]}};
      pub[0] = (u8)(2u | (y[0][0] & 1)), b32_bytes_of(pub + 1, &xs);
    }
    if (!b32_ckd(&k, c, path->el[d], pub)) return zero;
  }
  return k;
}
static bool seed_test_disagree(void) {
  const char *e = getenv("ECLOOP_HIP_TEST_SEED_DISAGREE");
  return e && e[0] == '1';
}
/* the found line of `mul` with two more fields: "addr33: <hash160> <- <key> <path> <phrase>"; in -o tab-separated, the phrase last */
static void seed_report(report_t *r, u8 type, const u32 *h, const sc *key, const char *path, const u8 *phrase, size_t plen) {
  char hh[67], kk[65];
  if (type == 5) snprintf(hh, 3, "%02x", 2u | (h[8] & 1u)), hex_of_words(hh + 2, h, 8);
  else hex_of_words(hh, h, type == 4 ? 8 : 5);
  hex_of_scalar(kk, key);
  const char *label = type == 5 ? "pub" : type == 4 ? "p2tr" : type == 3 ? "eth" : type == 2 ? "p2sh" : type ? "addr33" : "addr65";
  pthread_mutex_lock(&r->mu);
  if (!r->quiet) {
    erase_status_line();
    printf("%s: %s <- %s %s %.*s\n", label, hh, kk, path, (int)plen, (const char *)phrase);
    fflush(stdout);
  }
  if (r->file) fprintf(r->file, "%s\t%s\t%s\t%s\t%.*s\n", label, hh, kk, path, (int)plen, (const char *)phrase), fflush(r->file);
  r->found++;
  status_show_locked(r);
  pthread_mutex_unlock(&r->mu);
}
static void *seed_alloc(void *old, size_t bytes) { /* (re)allocation that ends the run with a message instead of returning NULL */
  void *p = realloc(old, bytes ? bytes : 1);
  if (!p) { fprintf(stderr, "seed: out of memory (%zu bytes)\n", bytes); exit(1); }
  return p;
}
/* stdin in chunks of at most SEED_CHUNK bytes, each ending behind a newline (or at the end of the input): an offset into a chunk always
   fits the 32 bits a line's table entry has for it, however long the input is.  What follows a chunk's last newline is carried to the
   front of the next one; a chunk without any newline (one line of 256 MiB and more) is handed out whole - it starts at a line's start
   or a multiple of 1024 bytes behind it, and SEED_CHUNK is a multiple of 1024, so the pieces of 1024 characters fall where they would. */
#define SEED_CHUNK ((size_t)256 << 20)
typedef struct { u8 *buf; size_t cap, have, used; bool eof; } seed_input;
static size_t seed_next_chunk(seed_input *in) { /* -> bytes of the chunk at in->buf, 0 at the end of the input */
  if (!in->buf) {
    /* test hook: ECLOOP_HIP_TEST_SEED_CHUNK=<KiB> reads in chunks of that many KiB, so that lines which end on, straddle and outgrow a
       chunk's end occur in an input of a few KiB (tests/test_seed_host.py) */
    const char *e = getenv("ECLOOP_HIP_TEST_SEED_CHUNK");
    const u64 kib = e ? strtoull(e, NULL, 10) : 0;
    in->cap = kib >= 1 && kib <= (SEED_CHUNK >> 10) ? (size_t)kib << 10 : SEED_CHUNK;
    in->buf = seed_alloc(NULL, in->cap);
  }
  memmove(in->buf, in->buf + in->used, in->have - in->used);
  in->have -= in->used, in->used = 0;
  while (!in->eof && in->have < in->cap) {
    const size_t got = fread(in->buf + in->have, 1, in->cap - in->have, stdin);
    if (!got) in->eof = true;
    in->have += got;
  }
  size_t n = in->have;
  if (!in->eof) /* (the buffer is full) */
    for (size_t e = in->have; e > 0; --e)
      if (in->buf[e - 1] == '\n') { n = e; break; }
  return in->used = n;
}
/* the non-empty lines of a chunk as `mul -raw` lists them: pieces of 1024 characters, '\r' before the newline dropped; entries are
   offset | length << 32 with offset < SEED_CHUNK < 2^32.  *table is grown as needed (*cap entries) */
static size_t seed_lines(const u8 *buf, size_t len, u64 **table, size_t *cap) {
  size_t n = 0, at = 0;
  while (at < len) {
    if (buf[at] == '\n') { /* empty lines: a run of newlines is stepped over eight at a time */
      u64 w;
      while (at + 8 <= len && (memcpy(&w, buf + at, 8), w == 0x0a0a0a0a0a0a0a0aULL)) at += 8;
      while (at < len && buf[at] == '\n') ++at;
      continue;
    }
    const u8 *nl = memchr(buf + at, '\n', len - at);
    const size_t stop = nl ? (size_t)(nl - buf) : len;
    for (size_t q = at; q < stop; q += MUL_LINE_MAX) {
      size_t l = stop - q < MUL_LINE_MAX ? stop - q : MUL_LINE_MAX;
      if (buf[q + l - 1] == '\r') l--;
      if (!l) continue;
      if (n == *cap) *cap = *cap ? *cap * 2 : 1 << 12, *table = seed_alloc(*table, *cap * 8);
      (*table)[n++] = (u64)q | (u64)l << 32;
    }
    at = stop + 1;
  }
  return n;
}

static int cmd_seed(run_t *run) {
  opts_t *o = &run->opt;
  /* ---- refusals, each by name, before a GPU is looked for */
  if (o->raw) seed_die("seed takes phrases, one per line: -raw%s does not go with it\n", "");
  if (o->bin) seed_die("seed takes phrases, one per line: -bin%s does not go with it\n", "");
  if (o->kdf) seed_die("seed derives keys by BIP39 / BIP32: -kdf %s does not go with it\n", o->kdf);
  if (o->prefix) seed_die("seed searches a list or a filter (-f): -p %s does not go with it\n", o->prefix);
  if (o->pubkey) seed_die("seed has no split-key form: -k %s does not go with it\n", o->pubkey);
  if (o->range) seed_die("seed has no range: -r %s does not go with it\n", o->range);
  if (opt_number(o->gpus, 1) > 1) seed_die("seed runs on one GPU: -t %s is not supported\n", o->gpus);
  seed_path paths[SEED_PATHS_MAX];
  int npaths = 0;
  if (o->path_missing) seed_die("-path needs a value%s\n", "");
  if (o->npaths > SEED_PATHS_MAX) seed_die("at most 8 -path options (at '%s')\n", o->paths[SEED_PATHS_MAX]);
  for (; npaths < o->npaths; ++npaths) {
    paths[npaths].depth = b32_parse_path(o->paths[npaths], paths[npaths].el);
    if (paths[npaths].depth < 0) seed_die("invalid -path '%s': m/44'/0'/0'/0/0 - numbers below 2^31, ' or h for hardened, at most 10 elements\n", o->paths[npaths]);
  }
  const u64 count = opt_number(o->count, 1);
  if (o->count && (count < 1 || count > SEED_COUNT_MAX || strspn(o->count, "0123456789") != strlen(o->count))) seed_die("invalid -n '%s': 1 ... 1024 values of each path's last element\n", o->count);
  const u8 *pass = (const u8 *)(o->pass ? o->pass : "");
  const size_t pass_len = strlen((const char *)pass);
  if (pass_len > B39_PASS_MAX) seed_die("invalid -pass: at most 99 bytes%s\n", "");
  run->a33 = o->addr ? strchr(o->addr, 'c') != NULL : true, run->a65 = o->addr && strchr(o->addr, 'u');
  if (run->eth || run->tr || run->pub) run->a33 = run->a65 = false;
  run->p2sh = o->addr && strchr(o->addr, 's');
  if (!run->a33 && !run->a65 && !run->p2sh && !run->eth && !run->tr && !run->pub) run->a33 = true;
  if (!npaths) { /* the default path by -a: BIP44, 49' for nested SegWit, 86' for Taproot, coin 60' for Ethereum */
    const char *def = run->eth ? "m/44'/60'/0'/0/0" : run->tr ? "m/86'/0'/0'/0/0" : (run->p2sh && !run->a33 && !run->a65) ? "m/49'/0'/0'/0/0" : "m/44'/0'/0'/0/0";
    paths[0].depth = b32_parse_path(def, paths[0].el), npaths = 1;
  }
  for (int p = 0; p < npaths; ++p) {
    if (count > 1 && !paths[p].depth) seed_die("-n %s needs a last element to count: not with the path m\n", o->count);
    if (count > 1 && (u64)(paths[p].el[paths[p].depth - 1] & ~B32_HARDENED) + count > B32_HARDENED) seed_die("-n %s: the last element of a path plus the count passes 2^31\n", o->count);
  }
  if (o->keys) { /* hidden: bip39_host.h alone, no GPU and no -f - the key of every line at every path of hardened elements */
    for (int p = 0; p < npaths; ++p)
      for (int d = 0; d < paths[p].depth; ++d)
        if (!(paths[p].el[d] & B32_HARDENED)) seed_die("seed -keys computes no public keys: every element of a path must be hardened%s\n", "");
    seed_input in = {0};
    u64 *lines = NULL;
    size_t cap = 0;
    for (size_t len; (len = seed_next_chunk(&in)) != 0;) {
      const size_t n = seed_lines(in.buf, len, &lines, &cap);
      for (size_t i = 0; i < n; ++i)
        for (int p = 0; p < npaths; ++p) {
          char kk[65];
          const sc k = seed_host_key(run, in.buf + (u32)lines[i], (size_t)(lines[i] >> 32), pass, pass_len, &paths[p]);
          hex_of_scalar(kk, &k);
          puts(kk);
        }
    }
    free(lines), free(in.buf);
    return 0;
  }
  if (o->quiet && !o->outfile) seed_die("quiet mode chosen without output file%s\n", "");
  filter_open(&run->flt, o->filter);
  if (ecl_hip_device_count() <= 0) { fprintf(stderr, "no MI355X GPU visible (the search path has no CPU fallback)\n"); return 1; }
  const u32 flags = (run->a33 ? ECL_ADDR33 : 0) | (run->a65 ? ECL_ADDR65 : 0) | (run->p2sh ? ECL_P2SH : 0) | (run->eth ? ECL_ETH : 0) | (run->tr ? ECL_TR : 0) |
                    (run->pub ? ECL_PUB : 0) | ECL_KDF_BIP39;
  run->cmd = CMD_MUL, run->ngpus = 1;
  int rc = ecl_hip_open(&run->dev[0], 0, flags, 0);
  if (rc == ECL_OK) rc = ecl_hip_set_bloom(run->dev[0], run->flt.words, run->flt.nwords);
  if (rc == ECL_OK && run->flt.list) rc = ecl_hip_set_list(run->dev[0], (const uint32_t(*)[5])run->flt.list, run->flt.nlist);
  if (rc != ECL_OK) die_ecl(run, 0, rc, "open");
  report_init(&run->rep, o->outfile, o->quiet);
  if (!o->quiet) printf("seed: %d path%s x %llu ~ filter: %s\n----------------------------------------\n", npaths, npaths == 1 ? "" : "s",
                        (unsigned long long)count, run->flt.list ? "list" : "bloom"), fflush(stdout);
  const bool disagree = seed_test_disagree();
  hits_t found = {NULL, 0}; /* kept, and what it grew to, across the calls */
  hits_room(&found, MUL_HITS_CAP);
  u64 *table = seed_alloc(NULL, ((size_t)SEED_BATCH + 1) * 8), *lines = NULL;
  u8 *text = NULL;
  size_t lines_cap = 0, text_cap = 0;
  seed_input in = {0};
  for (size_t len; (len = seed_next_chunk(&in)) != 0;) {
    const u8 *buf = in.buf;
    const size_t n = seed_lines(buf, len, &lines, &lines_cap);
    for (size_t at = 0; at < n; at += SEED_BATCH) {
      const u32 m = (u32)(n - at < SEED_BATCH ? n - at : SEED_BATCH);
      /* the batch's text: the record's slot, then the chunk from the first phrase of the batch to the end of its last (below 2^32 bytes:
         a chunk is) */
      const size_t first = (u32)lines[at], end = (u32)lines[at + m - 1] + (size_t)(lines[at + m - 1] >> 32);
      const size_t text_bytes = SEED_RECORD_ROOM + (end - first);
      if (text_bytes > text_cap) text = seed_alloc(text, text_cap = text_bytes);
      memcpy(text + SEED_RECORD_ROOM, buf + first, end - first);
      for (u32 i = 0; i < m; ++i) table[1 + i] = (u64)(SEED_RECORD_ROOM + ((u32)lines[at + i] - first)) | (lines[at + i] >> 32) << 32;
      bool fresh = true;
      for (int p = 0; p < npaths; ++p)
        for (u64 j = 0; j < count; ++j, fresh = false) {
          seed_path path = paths[p];
          if (path.depth) path.el[path.depth - 1] += (u32)j;
          char ptext[160];
          b32_format_path(ptext, sizeof ptext, path.el, path.depth);
          u8 *rec = text; /* "B39\0", reuse, depth, pass_len, 0; the elements, little-endian; the passphrase */
          memcpy(rec, "B39", 4), rec[4] = fresh ? 0 : 1, rec[5] = (u8)path.depth, rec[6] = (u8)pass_len, rec[7] = 0;
          for (int d = 0; d < path.depth; ++d) rec[8 + 4 * d] = (u8)path.el[d], rec[9 + 4 * d] = (u8)(path.el[d] >> 8), rec[10 + 4 * d] = (u8)(path.el[d] >> 16), rec[11 + 4 * d] = (u8)(path.el[d] >> 24);
          memcpy(rec + 8 + 4 * path.depth, pass, pass_len);
          table[0] = (u64)(8 + 4 * (size_t)path.depth + pass_len) << 32;
          u32 cnt = 0;
          do rc = ecl_hip_mul_batch_raw(run->dev[0], text, (u32)text_bytes, table, m + 1, found.rec, found.cap, &cnt);
          while (hits_need_repeat(run->dev[0], &rc, &found, cnt));
          if (rc != ECL_OK) die_ecl(run, 0, rc, "mul_batch_raw (seed)");
          const ecl_found *hits = found.rec;
          for (u32 i = 0; i < cnt; ++i) {
            if (!filter_confirms(&run->flt, hits[i].h160)) continue;
            const u64 ln = lines[at + hits[i].key_offset];
            sc pk = seed_host_key(run, buf + (u32)ln, (size_t)(ln >> 32), pass, pass_len, &path);
            /* test hook: ECLOOP_HIP_TEST_SEED_DISAGREE=1 flips the lowest bit of the host's key of every hit - what a device derivation that
               disagrees with the host's looks like from here - so that the verification below has to stop the run (tests/test_gpu_seed.py) */
            if (disagree) pk.w[0] ^= 1;
            u32 qx[1][FULL_WORDS];
            verify_hits(run, 0, &pk, &hits[i], 1, qx);
            seed_report(&run->rep, hits[i].compressed, run->tr || run->pub ? qx[0] : hits[i].h160, &pk, ptext, buf + (u32)ln, (size_t)(ln >> 32));
          }
          report_progress(&run->rep, m);
        }
    }
  }
  report_close(&run->rep);
  free(table), free(found.rec), free(lines), free(text), free(in.buf);
  ecl_hip_close(run->dev[0]);
  return 0;
}
