/* cli_splitkey.h - the split-key form of `-p` (add / rnd with -k <pubkey>) and the `combine` command (no reference counterpart).
   Part of the one translation unit ecloop_hip_cli.c (included there, in this order).  The arithmetic is host/splitkey.h's.
     searcher:   ecloop-hip add|rnd -p <pattern | file> -k <pubkey> [-a c|u|cu|e] [-endo] -r a:b
                 walks Q + k G on an ECL_PREFIX | ECL_ORIGIN context and prints PARTIAL keys: "addr33: <hash160> <- <partial key> <address> split:<e>"
     requester:  ecloop-hip combine -part <partial key> [-split <e>]   < their private key
                 prints the final key, calc_priv(k_Q, e) + partial (mod n) */
/* what -k cannot go with on add / rnd / mul; checked before anything is opened */
static void splitkey_check_options(const opts_t *o, const char *verb) {
  const bool add = !strcmp(verb, "add") || !strcmp(verb, "rnd");
  if (!strcmp(verb, "mul")) { fprintf(stderr, "-k is not supported with mul (a split-key search walks a range: add or rnd with -p)\n"); exit(1); }
  if (!add) return; /* bsgs, kangaroo: their own -k */
  if (o->filter) { fprintf(stderr, "-k and -f exclude each other: a split-key search goes with -p, which has no filter file\n"); exit(1); }
  if (!o->prefix) { fprintf(stderr, "-k goes with -p on %s: the split-key search for another person's public key is a prefix search\n", verb); exit(1); }
}
/* -k beside -p: exactly one public key (66 digits 02 / 03, 130 digits 04 on the curve; a bare x names two keys; a file of one key is
   taken, one of several is refused) */
static void splitkey_open(run_t *run, const char *arg) {
  size_t count = 0;
  bsgs_target *t = bsgs_targets(arg, &count);
  if (count != 1) { fprintf(stderr, "-k with -p takes one public key: '%s' holds %zu\n", arg, count); exit(1); }
  memcpy(run->origin, t->x, 32), memcpy(run->origin + 4, t->y, 32);
  memcpy(run->split_hex, t->hex, sizeof run->split_hex);
  run->split = true;
  free(t);
}

/* 1 ... 64 hex digits, nothing else (blanks around them are dropped; 0x in front is taken) -> the value; false otherwise */
static bool splitkey_hex(const char *s, bsgs_int *v) {
  while (isspace((unsigned char)*s)) ++s;
  if (s[0] == '0' && (s[1] | 0x20) == 'x') s += 2;
  size_t n = strlen(s);
  while (n && isspace((unsigned char)s[n - 1])) --n;
  if (!n || n > 64) return false;
  memset(v, 0, sizeof *v);
  for (size_t i = 0; i < n; ++i) {
    const int d = HEXVAL[(unsigned char)s[n - 1 - i]];
    if (d < 0) return false;
    v->w[i / 16] |= (u64)d << (4 * (i % 16));
  }
  return true;
}
static int cmd_combine(const opts_t *o) {
  bsgs_int part, kq;
  const bsgs_int zero = {{0, 0, 0, 0}};
  if (!o->part || !splitkey_hex(o->part, &part) || bsgs_cmp(&part, &BSGS_N) >= 0) {
    fprintf(stderr, "combine -part <partial key> [-split <e>]: the partial key is 1 ... 64 hex digits, below n\n");
    exit(1);
  }
  unsigned e = 0;
  if (o->split && (strlen(o->split) != 1 || o->split[0] < '0' || o->split[0] > '5')) {
    fprintf(stderr, "invalid -split '%s': the image of a found line, 0 ... 5\n", o->split);
    exit(1);
  }
  if (o->split) e = (unsigned)(o->split[0] - '0');
  char line[200];
  if (!fgets(line, sizeof line, stdin) || !splitkey_hex(line, &kq) || bsgs_cmp(&kq, &zero) == 0 || bsgs_cmp(&kq, &BSGS_N) >= 0) {
    fprintf(stderr, "combine reads the owner's private key from stdin: 1 ... 64 hex digits, 1 ... n - 1\n");
    exit(1);
  }
  const bsgs_int fin = sk_combine(kq, part, e);
  memset(line, 0, sizeof line), memset(&kq, 0, sizeof kq);
  if (bsgs_cmp(&fin, &zero) == 0) { fprintf(stderr, "the combined key is 0: no key (the partial key is not one of this key's)\n"); exit(1); }
  sc k;
  char kk[65];
  memcpy(k.w, fin.w, 32), hex_of_scalar(kk, &k);
  printf("key: %s\n", kk);
  fflush(stdout);
  if (ecl_hip_device_count() <= 0) return 0;
  /* the final key's addresses, by ecl_hip_verify on an ordinary context */
  ecl_hip *h = NULL;
  int rc = ecl_hip_open(&h, 0, ECL_ADDR33 | ECL_ADDR65, 0);
  u32 h33[1][5], h65[1][5], eth[1][5];
  u8 ok[2] = {0, 0};
  if (rc == ECL_OK) rc = ecl_hip_verify(h, (const uint64_t(*)[4])k.w, 1, h33, h65, ok);
  if (rc == ECL_OK) rc = ecl_hip_verify_eth(h, (const uint64_t(*)[4])k.w, 1, eth, ok + 1);
  if (rc != ECL_OK || !ok[0] || !ok[1]) bsgs_die(h, rc, "combine");
  char hh[41], a1[48], a2[48];
  hex_of_words(hh, h33[0], 5), pfx_address_b58(a1, h33[0]), pfx_address_bech32(a2, h33[0], 0);
  printf("addr33: %s %s %s\n", hh, a1, a2);
  hex_of_words(hh, h65[0], 5), pfx_address_b58(a1, h65[0]);
  printf("addr65: %s %s\n", hh, a1);
  hex_of_words(hh, eth[0], 5), pfx_address_eth(a1, eth[0]);
  printf("eth: %s %s\n", hh, a1);
  ecl_hip_close(h);
  return 0;
}
