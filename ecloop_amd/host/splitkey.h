/* splitkey.h - the arithmetic of the split-key vanity search (`-p` with `-k <pubkey>`, the `combine` command).  Plain C, no GPU: the CLI
   (cli_report.h, cli_splitkey.h) and the host test program (csrc/tools/splitkey_host.cpp) both include this file, so the code that is
   tested is the code that runs.

   The requester holds k_Q and sends Q = k_Q G.  The searcher walks P = Q + k G and reports k, the partial key: worthless without k_Q.
   With -endo the walk also probes the five other images of P under the curve's automorphisms - (x, -y), (beta x, +-y), (beta^2 x, +-y),
   numbered 0 ... 5 like the `endo` byte of a record (calc_priv, main.c:267-276: image e of k G has the key k, -k, lambda k, -lambda k,
   lambda^2 k, -lambda^2 k).  The automorphisms are group homomorphisms, so image e of P = Q + k G is O' + k' G with
     k' = calc_priv(k, e)                       (sk_endo_scalar: the partial key that is reported)
     O' = image e of Q                          (sk_image_origin: x times beta^(e / 2), y negated for odd e)
   and its private key is calc_priv(k_Q, e) + k' (mod n)   (sk_combine: what the requester computes; e = 0: k_Q + k). */
#ifndef SPLITKEY_H
#define SPLITKEY_H
#include "bsgs_plan.h" /* bsgs_int, the limb helpers and the field multiplication mod p (unsigned __int128) */

static const bsgs_int SK_LAMBDA = {{0xdf02967c1b23bd72ULL, 0x122e22ea20816678ULL, 0xa5261c028812645aULL, 0x5363ad4cc05c30e0ULL}};
static const uint64_t SK_BETA[4] = {0xc1396c28719501eeULL, 0x9cf0497512f58995ULL, 0x6e64479eac3434e9ULL, 0x7ae96a2b657c0710ULL};

/* ---- scalars mod n: canonical in (sk_modn_reduce brings any 256-bit value there), canonical out ---- */
static inline bsgs_int sk_modn_reduce(bsgs_int a) { /* a < 2^256 < 2 n */
  if (bsgs_cmp(&a, &BSGS_N) >= 0) bsgs_sub(&a, &a, &BSGS_N);
  return a;
}
static inline bsgs_int sk_modn_add(bsgs_int a, bsgs_int b) {
  bsgs_int r;
  const uint64_t c = bsgs_add(&r, &a, &b);
  if (c || bsgs_cmp(&r, &BSGS_N) >= 0) bsgs_sub(&r, &r, &BSGS_N);
  return r;
}
static inline bsgs_int sk_modn_neg(bsgs_int a) {
  bsgs_int r = {{0, 0, 0, 0}};
  if (a.w[0] | a.w[1] | a.w[2] | a.w[3]) bsgs_sub(&r, &BSGS_N, &a);
  return r;
}
static inline bsgs_int sk_modn_mul(bsgs_int a, bsgs_int b) { /* double-and-add: once per hit */
  bsgs_int r = {{0, 0, 0, 0}};
  for (int bit = 255; bit >= 0; --bit) {
    r = sk_modn_add(r, r);
    if ((b.w[bit >> 6] >> (bit & 63)) & 1) r = sk_modn_add(r, a);
  }
  return r;
}
/* calc_priv's endomorphism map (main.c:267-276) of a key: e = 0 ... 5 */
static inline bsgs_int sk_endo_scalar(bsgs_int k, unsigned e) {
  k = sk_modn_reduce(k);
  if (e == 2 || e == 3) k = sk_modn_mul(k, SK_LAMBDA);
  if (e == 4 || e == 5) k = sk_modn_mul(sk_modn_mul(k, SK_LAMBDA), SK_LAMBDA);
  if (e & 1) k = sk_modn_neg(k);
  return k;
}
/* image e of the affine point (x, y), in place: x times beta^(e / 2), y negated for odd e (canonical limbs in and out) */
static inline void sk_image_origin(uint64_t x[4], uint64_t y[4], unsigned e) {
  for (unsigned j = 0; j < e / 2; ++j) bsgs_fp_mul(x, x, SK_BETA);
  if (e & 1) bsgs_fp_neg(y, y);
}
/* the requester's final key for a partial key reported with image e: calc_priv(k_Q, e) + partial (mod n) */
static inline bsgs_int sk_combine(bsgs_int kq, bsgs_int partial, unsigned e) { return sk_modn_add(sk_endo_scalar(kq, e), sk_modn_reduce(partial)); }
#endif
