/* cli_brain.h - `brain` (no reference counterpart): pass phrases generated on the device from a template -> their hash -> the address
   search of `mul -raw`.
     ecloop-hip brain -f <list | .blf> -mask <template> [-1 <set>] ... [-4 <set>] [-a ...] [-kdf sha256|keccak|sha3|camp2] [-r a:b] [-o file] [-q]
   The template and the order of its candidates are defined in gen_plan.h (the mask's classes, the sets, @file word lists).  A candidate
   is a 64-bit index; -r a:b (hex, both ends included) searches a part of 0 ... T - 1, and the status line shows the index reached and T,
   so a run is resumed with -r.  Calls of 2^24 candidates on a context opened with ECL_GEN (include/ecloop_hip.h): the template crosses
   to the device once, then one index per call.  Every hit of every type and every -kdf is verified: the phrase is generated again here
   from the index (gen_candidate_host: division and remainder, not the device's odometer), hashed with raw_line_digest, and the hit is
   re-derived on the device from that key (verify_hits) - a generator that disagreed ends the run with the hash mismatch error.
   Part of the one translation unit ecloop_hip_cli.c. */
#define BRAIN_CALL (1u << 24)

static void brain_die(const char *fmt, const char *arg) {
  fprintf(stderr, fmt, arg);
  exit(1);
}
static bool brain_test_disagree(void) {
  const char *e = getenv("ECLOOP_HIP_TEST_BRAIN_DISAGREE");
  return e && e[0] == '1';
}
/* up to 16 hex digits, nothing else: false otherwise */
static bool brain_hex64(const char *s, size_t n, u64 *v) {
  if (n < 1 || n > 16) return false;
  *v = 0;
  for (size_t i = 0; i < n; ++i) {
    const char c = s[i];
    const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
    if (d < 0) return false;
    *v = *v << 4 | (u64)d;
  }
  return true;
}
/* the found line of `mul` with two more fields: "addr33: <hash160> <- <key> <index hex> <phrase>"; in -o tab-separated, the phrase last */
static void brain_report(report_t *r, u8 type, const u32 *h, const sc *key, u64 index, const u8 *phrase, size_t plen) {
  char hh[67], kk[65];
  if (type == 5) snprintf(hh, 3, "%02x", 2u | (h[8] & 1u)), hex_of_words(hh + 2, h, 8);
  else hex_of_words(hh, h, type == 4 ? 8 : 5);
  hex_of_scalar(kk, key);
  const char *label = type == 5 ? "pub" : type == 4 ? "p2tr" : type == 3 ? "eth" : type == 2 ? "p2sh" : type ? "addr33" : "addr65";
  pthread_mutex_lock(&r->mu);
  if (!r->quiet) {
    erase_status_line();
    printf("%s: %s <- %s %llx ", label, hh, kk, (unsigned long long)index);
    fwrite(phrase, 1, plen, stdout);
    putchar('\n');
    fflush(stdout);
  }
  if (r->file) {
    fprintf(r->file, "%s\t%s\t%s\t%llx\t", label, hh, kk, (unsigned long long)index);
    fwrite(phrase, 1, plen, r->file);
    fputc('\n', r->file), fflush(r->file);
  }
  r->found++;
  status_show_locked(r);
  pthread_mutex_unlock(&r->mu);
}

static int cmd_brain(run_t *run) {
  opts_t *o = &run->opt;
  /* ---- refusals, each by name, before a GPU is looked for */
  if (o->raw) brain_die("brain generates its phrases: -raw%s does not go with it\n", "");
  if (o->bin) brain_die("brain generates its phrases: -bin%s does not go with it\n", "");
  if (o->prefix) brain_die("brain searches a list or a filter (-f): -p %s does not go with it\n", o->prefix);
  if (o->pubkey) brain_die("brain has no split-key form: -k %s does not go with it\n", o->pubkey);
  if (o->npaths || o->path_missing) brain_die("brain hashes a phrase once (see `seed` for BIP39): -path%s does not go with it\n", "");
  if (o->pass) brain_die("brain hashes a phrase once (see `seed` for BIP39): -pass %s does not go with it\n", o->pass);
  if (opt_number(o->gpus, 1) > 1) brain_die("brain runs on one GPU: -t %s is not supported\n", o->gpus);
  run->kdf = KDF_SHA256;
  if (o->kdf && (run->kdf = kdf_from_name(o->kdf)) < 0) brain_die("invalid -kdf '%s': one of sha256, keccak, sha3, camp2\n", o->kdf);
  if (!o->mask) brain_die("brain needs a template: -mask <template>%s (?l ?u ?d ?h ?s ?a, ?1 ... ?4 with -1 ... -4 <set | @file>, ?? for a '?')\n", "");
  char why[320];
  gen_build sets[4], built;
  const gen_build *use[4] = {NULL, NULL, NULL, NULL};
  for (int k = 0; k < 4; ++k)
    if (o->set[k]) {
      if (gen_parse_set(o->set[k], (char)('1' + k), &sets[k], why, sizeof why)) brain_die("invalid %s\n", why);
      use[k] = &sets[k];
    }
  if (gen_parse_mask(o->mask, use, &built, why, sizeof why)) brain_die("%s\n", why);
  size_t blob_bytes = 0;
  u8 *blob = gen_build_blob(&built, &blob_bytes);
  if (!blob) brain_die("brain: out of memory for the template%s\n", "");
  for (int k = 0; k < 4; ++k)
    if (use[k]) gen_build_free(&sets[k]);
  gen_build_free(&built);
  gen_info gi;
  const char *bad = gen_blob_check(blob, blob_bytes, &gi);
  if (bad) brain_die("invalid -mask: %s\n", bad);
  u64 a = 0, b = gi.T - 1;
  if (o->range) {
    const char *colon = strchr(o->range, ':');
    if (!colon || !brain_hex64(o->range, (size_t)(colon - o->range), &a) || !brain_hex64(colon + 1, strlen(colon + 1), &b))
      brain_die("invalid -r '%s': candidate indices a:b in hex, both ends included\n", o->range);
    if (a > b) brain_die("invalid -r '%s': a is above b\n", o->range);
    if (b >= gi.T) {
      fprintf(stderr, "invalid -r '%s': the template has %llx candidates, 0 ... %llx\n", o->range, (unsigned long long)gi.T, (unsigned long long)(gi.T - 1));
      exit(1);
    }
  }
  u8 phrase[GEN_L_MAX];
  if (o->keys) { /* hidden: gen_plan.h and the host's hashes alone, no GPU and no -f - index, phrase and digest of every candidate of -r */
    for (u64 i = a;; ++i) {
      const u32 len = gen_candidate_host(blob, &gi, i, phrase);
      u32 st[8];
      char hh[65];
      raw_line_digest(run, st, phrase, len);
      hex_of_words(hh, st, 8);
      printf("%llx\t", (unsigned long long)i);
      fwrite(phrase, 1, len, stdout);
      printf("\t%s\n", hh);
      if (i == b) break;
    }
    free(blob);
    return 0;
  }
  run->a33 = o->addr ? strchr(o->addr, 'c') != NULL : true, run->a65 = o->addr && strchr(o->addr, 'u');
  if (run->eth || run->tr || run->pub) run->a33 = run->a65 = false;
  run->p2sh = o->addr && strchr(o->addr, 's');
  if (!run->a33 && !run->a65 && !run->p2sh && !run->eth && !run->tr && !run->pub) run->a33 = true;
  if (o->quiet && !o->outfile) brain_die("quiet mode chosen without output file%s\n", "");
  filter_open(&run->flt, o->filter);
  if (ecl_hip_device_count() <= 0) { fprintf(stderr, "no MI355X GPU visible (the search path has no CPU fallback)\n"); return 1; }
  const u32 flags = (run->a33 ? ECL_ADDR33 : 0) | (run->a65 ? ECL_ADDR65 : 0) | (run->p2sh ? ECL_P2SH : 0) | (run->eth ? ECL_ETH : 0) | (run->tr ? ECL_TR : 0) |
                    (run->pub ? ECL_PUB : 0) | ECL_GEN |
                    (run->kdf == KDF_KECCAK ? ECL_KDF_KECCAK : run->kdf == KDF_SHA3 ? ECL_KDF_SHA3 : run->kdf == KDF_CAMP2 ? ECL_KDF_CAMP2 : 0);
  run->cmd = CMD_MUL, run->ngpus = 1;
  int rc = ecl_hip_open(&run->dev[0], 0, flags, 0);
  if (rc == ECL_OK) rc = ecl_hip_set_bloom(run->dev[0], run->flt.words, run->flt.nwords);
  if (rc == ECL_OK && run->flt.list) rc = ecl_hip_set_list(run->dev[0], (const uint32_t(*)[5])run->flt.list, run->flt.nlist);
  if (rc != ECL_OK) die_ecl(run, 0, rc, "open");
  report_init(&run->rep, o->outfile, o->quiet);
  run->rep.brain = true, run->rep.brain_at = a, run->rep.brain_T = gi.T;
  if (!o->quiet) printf("brain: %u position%s, %llx candidates, %llx ... %llx ~ kdf: %s ~ filter: %s\n----------------------------------------\n", gi.npos,
                        gi.npos == 1 ? "" : "s", (unsigned long long)gi.T, (unsigned long long)a, (unsigned long long)b, KDF_NAMES[run->kdf],
                        run->flt.list ? "list" : "bloom"), fflush(stdout);
  const bool disagree = brain_test_disagree();
  hits_t found = {NULL, 0};
  hits_room(&found, MUL_HITS_CAP);
  for (u64 at = a;;) {
    const u64 left = b - at + 1; /* (0 stands for 2^64: the whole of a template of 2^64 - 1 candidates never gets here - T < 2^64 and b < T) */
    const u32 n = left < BRAIN_CALL ? (u32)left : BRAIN_CALL;
    u32 cnt = 0;
    do rc = ecl_hip_mul_batch_raw(run->dev[0], blob, (u32)blob_bytes, &at, n, found.rec, found.cap, &cnt);
    while (hits_need_repeat(run->dev[0], &rc, &found, cnt));
    if (rc != ECL_OK) die_ecl(run, 0, rc, "mul_batch_raw (brain)");
    const ecl_found *hits = found.rec;
    for (u32 i = 0; i < cnt; ++i) {
      if (!filter_confirms(&run->flt, hits[i].h160)) continue;
      const u64 index = at + hits[i].key_offset;
      /* test hook: ECLOOP_HIP_TEST_BRAIN_DISAGREE=1 makes the host generate the candidate behind the hit's (the first one behind the last)
         - what a device generator that disagrees with the host's looks like from here - so that the verification below has to stop the run
         (tests/test_gpu_brain.py) */
      const u32 len = gen_candidate_host(blob, &gi, disagree ? (index + 1 < gi.T ? index + 1 : 0) : index, phrase);
      u32 st[8];
      raw_line_digest(run, st, phrase, len);
      const sc pk = {{(u64)st[6] << 32 | st[7], (u64)st[4] << 32 | st[5], (u64)st[2] << 32 | st[3], (u64)st[0] << 32 | st[1]}};
      u32 qx[1][FULL_WORDS];
      verify_hits(run, 0, &pk, &hits[i], 1, qx);
      brain_report(&run->rep, hits[i].compressed, run->tr || run->pub ? qx[0] : hits[i].h160, &pk, index, phrase, len);
    }
    pthread_mutex_lock(&run->rep.mu);
    run->rep.brain_at = at + (n - 1); /* the last index searched: -r <that + 1>:... goes on from here */
    pthread_mutex_unlock(&run->rep.mu);
    report_progress(&run->rep, n);
    if (left == n) break;
    at += n;
  }
  report_close(&run->rep);
  free(found.rec), free(blob);
  ecl_hip_close(run->dev[0]);
  return 0;
}
