/* cli_prefix.h - `-p`: the prefix (vanity) search of `add` / `rnd` - patterns from the command line or a file, the plan (prefix_plan.h)
   as the run's filter, and the found line of a hit with its address.
   Part of the one translation unit ecloop_hip_cli.c (included there, in this order). */
/* -p <pattern | file of patterns>: a name that opens as a file is a list, one pattern per line (blank lines skipped); anything else is
   the pattern itself.  The planned table stands where the bloom words of -f stand (run->flt.words: ten 32-bit words per range), so the
   bring-up hands it to ecl_hip_set_bloom of a context opened with ECL_PREFIX.  A list with a 0x pattern that has ? or * (a suffix, both
   ends, holes) is planned by mask_plan.h instead: its mask table stands in the same place and the context is opened with ECL_MASK. */
static void prefix_open(run_t *run, const char *arg) {
  char **pats = NULL;
  u32 n = 0;
  FILE *in = fopen(arg, "rb");
  if (in) {
    size_t len;
    char *text = slurp(in, &len);
    fclose(in);
    text = realloc(text, len + 1), text[len] = 0;
    for (char *line = strtok(text, "\r\n"); line; line = strtok(NULL, "\r\n")) {
      while (*line == ' ' || *line == '\t') ++line;
      char *end = line + strlen(line);
      while (end > line && (end[-1] == ' ' || end[-1] == '\t')) *--end = 0;
      if (!*line) continue;
      pats = realloc(pats, sizeof *pats * (n + 1)), pats[n++] = line;
    }
    if (!n) { fprintf(stderr, "no patterns in file: %s\n", arg); exit(1); }
  } else {
    pats = malloc(sizeof *pats), pats[0] = (char *)arg, n = 1;
  }
  static pfx_plan plan;
  char why[320];
  if (msk_list_is_masked((const char *const *)pats, n)) {
    static msk_plan mplan;
    if (msk_plan_make(&mplan, (const char *const *)pats, n, run->eth, why, sizeof why) != PFX_OK) {
      fprintf(stderr, "%s\n", why);
      exit(1);
    }
    free(pats);
    memset(&plan, 0, sizeof plan);
    plan.pat = mplan.pat, plan.npat = mplan.npat; /* (the patterns alone: a run with -p has run->pfx set) */
    run->pfx = &plan, run->msk = &mplan;
    memset(&run->flt, 0, sizeof run->flt);
    run->flt.nwords = 5ull * mplan.nentry;
    run->flt.words = malloc(run->flt.nwords * 8);
    memcpy(run->flt.words, mplan.entry, run->flt.nwords * 8); /* msk_entry is m[5], v[5]: the table's layout */
    return;
  }
  if (pfx_plan_make(&plan, (const char *const *)pats, n, run->a33, run->a65, run->eth, why, sizeof why) != PFX_OK) {
    fprintf(stderr, "%s\n", why);
    exit(1);
  }
  free(pats);
  run->pfx = &plan;
  memset(&run->flt, 0, sizeof run->flt);
  run->flt.nwords = 5ull * plan.nrange;
  run->flt.words = malloc(run->flt.nwords * 8);
  memcpy(run->flt.words, plan.range, run->flt.nwords * 8); /* pfx_range is lo[5], hi[5]: the table's layout */
}
/* what -p cannot go with; checked before anything is opened */
static void prefix_check_options(const opts_t *o, const char *verb) {
  if (o->filter) { fprintf(stderr, "-p and -f exclude each other: a prefix search has no filter file\n"); exit(1); }
  if (!strcmp(verb, "mul")) { fprintf(stderr, "-p is not supported with mul (prefix search walks a range: add or rnd)\n"); exit(1); }
  if (strcmp(verb, "add") && strcmp(verb, "rnd")) { fprintf(stderr, "-p goes with add or rnd\n"); exit(1); }
  if (o->addr && strpbrk(o->addr, "stx")) {
    fprintf(stderr, "-p is not supported with -a %s: prefix patterns are 1... (-a c, u, cu), bc1q... (-a c) and 0x... (-a e)\n", o->addr);
    exit(1);
  }
}
/* the hits of one device call, verified already: each one's address text against the patterns.  A record that matches none is a range's
   end value whose checksum does not fit: dropped and counted (the status line shows the count).  The found line is the sink's with the
   address appended: "addr33: <hash160> <- <key> <address>" on stdout, a fourth tab-separated field in the -o file.  A split-key run
   (-k) prints the partial key there and one more field, split:<e> - the image the requester's `combine` needs */
static void prefix_report(run_t *run, const ecl_found *hits, const sc *keys, u32 n) {
  report_t *r = &run->rep;
  for (u32 i = 0; i < n; ++i) {
    char addr[48], hh[41], kk[65], sp[16] = "", spf[16] = "";
    if (run->msk) { /* the mask test is exact: a record that matches no pattern is an error, not an edge */
      if (msk_match(run->msk, hits[i].h160, addr) < 0) {
        fprintf(stderr, "[!] error: the record %s matches no pattern\n", addr);
        exit(1);
      }
    } else if (pfx_match(run->pfx, hits[i].h160, hits[i].compressed, addr) < 0) {
      pthread_mutex_lock(&r->mu);
      r->edge++;
      pthread_mutex_unlock(&r->mu);
      continue;
    }
    hex_of_words(hh, hits[i].h160, 5), hex_of_scalar(kk, &keys[i]);
    const char *label = hits[i].compressed == 3 ? "eth" : hits[i].compressed ? "addr33" : "addr65";
    if (run->split) snprintf(sp, sizeof sp, " split:%u", hits[i].endo), snprintf(spf, sizeof spf, "\tsplit:%u", hits[i].endo);
    pthread_mutex_lock(&r->mu);
    if (!r->quiet) erase_status_line(), printf("%s: %s <- %s %s%s\n", label, hh, kk, addr, sp), fflush(stdout);
    if (r->file) fprintf(r->file, "%s\t%s\t%s\t%s%s\n", label, hh, kk, addr, spf), fflush(r->file);
    r->found++;
    status_show_locked(r);
    pthread_mutex_unlock(&r->mu);
  }
}
