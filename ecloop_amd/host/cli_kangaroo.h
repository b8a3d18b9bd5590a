/* cli_kangaroo.h - the `kangaroo` command: Pollard's lambda search for the private key of a KNOWN public key in a range (no reference
   counterpart).  Part of the one translation unit ecloop_hip_cli.c (included there, after cli_bsgs.h: -k and -r are read by its functions).
   The method and its arithmetic are host/kangaroo_plan.h's; here: the command line, the one device context (ECL_PUB | ECL_HERD), the store
   of distinguished points and the resolution of collisions.
     ecloop-hip kangaroo -k <pubkey | file of pubkeys> -r a:b [-herd log2] [-dp bits] [-seed s] [-max factor] [-o file] [-q]
   Targets are searched one after another, each from scratch.  A round is one ecl_hip_add_range; its records are sorted by (identity,
   distance, herd) and put into an open-addressing table keyed on the 96-bit identity.  A tame / wild pair gives two candidate keys, each
   re-derived with ecl_hip_diag_mulg and accepted only if all 32 bytes of x and the parity of y are the target's.  One GPU. */
#include "kangaroo_plan.h"

typedef struct { u64 id_lo, d_lo, d_hi; u32 id_hi; u8 herd, used; } kg_slot;
typedef struct { kg_slot *slot; u64 mask, count; } kg_store;

static u64 kg_hash(u64 id_lo, u32 id_hi) {
  u64 z = id_lo ^ ((u64)id_hi * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  return z ^ (z >> 27);
}
static void kg_store_init(kg_store *s, u64 slots) {
  s->slot = calloc(slots, sizeof *s->slot), s->mask = slots - 1, s->count = 0;
  if (!s->slot) { fprintf(stderr, "\n[!] kangaroo: out of memory for the point store\n"); exit(1); }
}
/* the slot of an identity: the one that holds it, or the free one where it goes */
static kg_slot *kg_store_find(kg_store *s, u64 id_lo, u32 id_hi) {
  for (u64 at = kg_hash(id_lo, id_hi) & s->mask;; at = (at + 1) & s->mask) {
    kg_slot *e = &s->slot[at];
    if (!e->used || (e->id_lo == id_lo && e->id_hi == id_hi)) return e;
  }
}
static void kg_store_grow(kg_store *s) {
  kg_store big;
  kg_store_init(&big, 2 * (s->mask + 1));
  for (u64 i = 0; i <= s->mask; ++i)
    if (s->slot[i].used) *kg_store_find(&big, s->slot[i].id_lo, s->slot[i].id_hi) = s->slot[i];
  big.count = s->count;
  free(s->slot);
  *s = big;
}
static u64 kg_id_lo(const ecl_found *r) { return (u64)r->h160[3] << 32 | r->h160[4]; }
static u64 kg_d_hi(const ecl_found *r) { return (u64)r->h160[0] << 32 | r->h160[1]; }
static int kg_order(const void *p, const void *q) { /* (identity, distance, herd) */
  const ecl_found *a = p, *b = q;
  if (a->h160[2] != b->h160[2]) return a->h160[2] < b->h160[2] ? -1 : 1;
  if (kg_id_lo(a) != kg_id_lo(b)) return kg_id_lo(a) < kg_id_lo(b) ? -1 : 1;
  if (kg_d_hi(a) != kg_d_hi(b)) return kg_d_hi(a) < kg_d_hi(b) ? -1 : 1;
  if (a->key_offset != b->key_offset) return a->key_offset < b->key_offset ? -1 : 1;
  return (int)a->endo - (int)b->endo;
}
static void kg_status(bool quiet, u128 jumps, u64 dps, u64 same, bool last) {
  if (quiet) return;
  erase_status_line();
  if (jumps >> 64) fprintf(stderr, "jumps: 2^%u", 128 - (unsigned)__builtin_clzll((u64)(jumps >> 64)));
  else fprintf(stderr, "jumps: %'llu", (unsigned long long)jumps);
  fprintf(stderr, " ~ distinguished points: %'llu ~ same-herd collisions: %'llu%c", (unsigned long long)dps, (unsigned long long)same, last ? '\n' : '\r');
  fflush(stderr);
}
static bool kg_all_digits(const char *s) { return s && *s && strspn(s, "0123456789") == strlen(s); }

static int cmd_kangaroo(const opts_t *o) {
  if (opt_number(o->gpus, 1) > 1) { fprintf(stderr, "kangaroo runs on one GPU: -t %s is not supported\n", o->gpus); exit(1); }
  if (!o->pubkey) { fprintf(stderr, "kangaroo: missing -k <pubkey | file of pubkeys>\n"); exit(1); }
  if (o->quiet && !o->outfile) { fprintf(stderr, "quiet mode chosen without output file\n"); exit(1); }
  bsgs_int a, b;
  bsgs_range(o->range, &a, &b);
  if (o->herd && (!kg_all_digits(o->herd) || opt_number(o->herd, 0) < 1 || opt_number(o->herd, 0) > KG_HERD_LOG2_MAX)) {
    fprintf(stderr, "invalid -herd '%s': the herd is 2^herd kangaroos, herd = 1 ... %u\n", o->herd, KG_HERD_LOG2_MAX);
    exit(1);
  }
  if (o->dp && (!kg_all_digits(o->dp) || opt_number(o->dp, 0) > KG_DP_MAX)) {
    fprintf(stderr, "invalid -dp '%s': the distinguished-point bits, 0 ... %u\n", o->dp, KG_DP_MAX);
    exit(1);
  }
  if (o->maxf && (!kg_all_digits(o->maxf) || !opt_number(o->maxf, 0) || opt_number(o->maxf, 0) > 0xFFFFFFFFull)) {
    fprintf(stderr, "invalid -max '%s': the give-up limit is max * 2 sqrt(range) jumps, max = 1 ... 2^32 - 1\n", o->maxf);
    exit(1);
  }
  const u64 seed = o->seed ? strtoull(o->seed, NULL, 0) : 0;
  const u32 max_factor = (u32)opt_number(o->maxf, 64);
  kg_plan plan;
  const int prc = kg_plan_make(&plan, &a, &b, o->herd ? (int)opt_number(o->herd, 0) : -1, o->dp ? (int)opt_number(o->dp, 0) : -1);
  if (prc == KG_E_ORDER) { fprintf(stderr, "invalid search range: kangaroo needs 1 <= a <= b < n\n"); exit(1); }
  if (prc == KG_E_WIDTH) { fprintf(stderr, "invalid search range: more than 2^124 keys\n"); exit(1); }
  if (prc != KG_OK) { fprintf(stderr, "invalid options\n"); exit(1); }
  size_t ntargets = 0;
  bsgs_target *targets = bsgs_targets(o->pubkey, &ntargets);
  if (ecl_hip_device_count() <= 0) { fprintf(stderr, "no MI355X GPU visible (the search path has no CPU fallback)\n"); return 1; }
  FILE *outfile = o->outfile ? fopen(o->outfile, "a") : NULL;
  ecl_hip *h = NULL;
  int rc = ecl_hip_open(&h, 0, ECL_PUB | ECL_HERD, plan.dp);
  if (rc != ECL_OK) bsgs_die(h, rc, "herd context");
  const u64 H = 1ull << plan.herd_log2, round_jumps = plan.round_steps * H;
  const kg_u128 lim = kg_give_up(&plan, max_factor);
  const u128 limit = (u128)lim.hi << 64 | lim.lo;
  if (!o->quiet) {
    printf("kangaroo: %zu target%s ~ range: 2^%u keys ~ herd: 2^%u ~ dp: %u ~ jump bits: %u ~ round: %'llu jumps\n----------------------------------------\n",
           ntargets, ntargets == 1 ? "" : "s", plan.wbits, plan.herd_log2, plan.dp, plan.jb, (unsigned long long)round_jumps);
    fflush(stdout);
  }
  /* records of a round: twice the expected number and some, the rest of a fuller round comes through hits_need_repeat */
  hits_t hits = {NULL, 0}; /* kept, and what it grew to, across the rounds and the targets */
  hits_room(&hits, (round_jumps >> plan.dp) > (1ull << 26) ? 1u << 27 : (u32)(2 * (round_jumps >> plan.dp) + 4096));
  for (size_t t = 0; t < ntargets; ++t) {
    const bsgs_target *q = &targets[t];
    u64 blk[16];
    kg_block(blk, &plan, q->x, q->y, seed);
    kg_store store;
    kg_store_init(&store, 1ull << 16);
    u128 jumps = 0;
    u64 same = 0;
    bool found = false;
    while (!found) {
      u32 n = 0;
      rc = ecl_hip_add_range(h, blk, round_jumps, hits.rec, hits.cap, &n);
      if (hits_need_repeat(h, &rc, &hits, n)) { /* (too few -dp bits; the round is not made again) */
        fprintf(stderr, "\n[!] kangaroo: more records in one round than the device keeps; use more -dp bits\n");
        exit(1);
      }
      if (rc != ECL_OK) bsgs_die(h, rc, "herd");
      ecl_found *recs = hits.rec;
      jumps += round_jumps;
      qsort(recs, n, sizeof *recs, kg_order);
      for (u32 r = 0; r < n && !found; ++r) {
        if (2 * (store.count + 1) > store.mask) kg_store_grow(&store);
        kg_slot *e = kg_store_find(&store, kg_id_lo(&recs[r]), recs[r].h160[2]);
        if (!e->used) {
          e->used = 1, e->herd = recs[r].endo, e->id_lo = kg_id_lo(&recs[r]), e->id_hi = recs[r].h160[2];
          e->d_lo = recs[r].key_offset, e->d_hi = kg_d_hi(&recs[r]);
          ++store.count;
          continue;
        }
        if (e->herd == recs[r].endo) { ++same; continue; }
        const kg_u128 de = {e->d_lo, e->d_hi}, dr = {recs[r].key_offset, kg_d_hi(&recs[r])};
        bsgs_int cand[2];
        kg_candidates(&cand[0], &cand[1], &plan.base, e->herd ? dr : de, e->herd ? de : dr);
        for (int c = 0; c < 2 && !found; ++c) {
          u64 x[1][4], y[1][4];
          u8 fin = 0;
          rc = ecl_hip_diag_mulg(h, (const uint64_t(*)[4])cand[c].w, x, y, &fin, 1);
          if (rc != ECL_OK) bsgs_die(h, rc, "verify");
          if (fin && !memcmp(x[0], q->x, 32) && (y[0][0] & 1) == (q->y[0] & 1)) {
            bsgs_found(outfile, o->quiet, q->hex, &cand[c]);
            found = true;
          }
        }
      }
      kg_status(o->quiet, jumps, store.count, same, false);
      if (!found && jumps >= limit) break;
    }
    kg_status(o->quiet, jumps, store.count, same, true);
    if (!found) {
      if (jumps >> 64) fprintf(stderr, "%s not found within 2^%u jumps\n", q->hex, 128 - (unsigned)__builtin_clzll((u64)(jumps >> 64)));
      else fprintf(stderr, "%s not found within %llu jumps\n", q->hex, (unsigned long long)jumps);
    }
    free(store.slot);
  }
  free(hits.rec), free(targets);
  if (outfile) fclose(outfile);
  ecl_hip_close(h);
  return 0;
}
