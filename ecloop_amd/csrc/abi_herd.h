// abi_herd.h - host side of ECL_PUB | ECL_HERD: the herd of `kangaroo` behind ecl_hip_add_range (herd_kernel.h has the kernels,
// host/kangaroo_plan.h the method).  (one translation unit: included by ecloop_hip.hip)
#pragma once
#include "../host/kangaroo_plan.h"

#define HERD_INIT_CHUNK (1u << 18)     /* kangaroos whose starts are multiplied per set-up launch */
#define HERD_LAUNCH_STEPS_MAX 4096u    /* steps of one launch: a lone wave makes a step of 32 jumps in a fraction of a millisecond ... */
#define HERD_LAUNCH_JUMPS_LOG2 34u     /* ... and a full chip is given at most 2^34 jumps per launch (static estimates) */

struct herd_params {
  u256 base;
  u32 q[16];  // canonical words x[8], y[8]
  u64 seed;
  u32 herd_log2, jb, sb;
};
// the sixteen limbs of `start`, checked: ECL_E_ARG with the reason in h->err
static int herd_parse(ecl_hip* h, const uint64_t blk[16], herd_params& p) {
  p.base = sc_reduce(u256_from(blk));
  if (!origin_from_limbs(p.q, blk + 4)) {
    h->err = "the target is not a point of the curve";
    return ECL_E_ARG;
  }
  p.seed = blk[12];
  if (blk[13] < 1 || blk[13] > KG_HERD_LOG2_MAX || blk[14] < KG_JB_MIN || blk[14] > KG_JB_MAX || blk[15] < 1 || blk[15] > KG_SB_MAX) {
    h->err = "herd block: herd_log2 1 ... 24, jump_bits 4 ... 120, spread_bits 1 ... 124";
    return ECL_E_ARG;
  }
  p.herd_log2 = (u32)blk[13], p.jb = (u32)blk[14], p.sb = (u32)blk[15];
  return ECL_OK;
}

// table and starts of a new herd, queued on h->stream and waited for; the flag word CW_HERD_FLAGS (zeroed by the caller) comes home in *flags
static int herd_build(ecl_hip* h, const herd_params& p, u32* flags) {
  const u32 H = 1u << p.herd_log2;
  HIPCHK(h, h->d_herd.grow((size_t)H * 22));  // (every launch on the herd was waited for by its call's read-back)
  HIPCHK(h, h->d_herdtab.grow(32 * HERD_TAB_IN));
  kg_stream st = {p.seed};
  kg_u128 s[KG_TABLE];
  kg_table(&st, p.jb, s);
  const u32 chunk = H < HERD_INIT_CHUNK ? H : HERD_INIT_CHUNK, nk = chunk > 32 ? chunk : 32;
  devbuf<u32> d_k, d_pts, d_r;
  devbuf<u8> d_ok;
  HIPCHK(h, d_k.grow((size_t)nk * 8));
  HIPCHK(h, d_pts.grow((size_t)nk * 16));
  HIPCHK(h, d_r.grow((size_t)chunk * 4));
  HIPCHK(h, d_ok.grow(nk));
  std::vector<u32> ks((size_t)nk * 8), rs((size_t)chunk * 4), tab(32 * HERD_TAB_IN);
  // T_j = s_j G by the double-and-add kernel
  for (u32 j = 0; j < 32; ++j) {
    const uint64_t w[4] = {s[j].lo, s[j].hi, 0, 0};
    words_of(&ks[(size_t)j * 8], u256_from(w));
  }
  HIPCHK(h, hipMemcpyAsync(d_k.p, ks.data(), 32 * 8 * sizeof(u32), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_mul_g, dim3(1), dim3(64), 0, h->stream, d_k.p, d_pts.p, d_ok.p, 32u);
  HIPCHK(h, hipGetLastError());
  std::vector<u32> tpts(32 * 16);
  HIPCHK(h, hipMemcpyAsync(tpts.data(), d_pts.p, tpts.size() * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (u32 j = 0; j < 32; ++j) {
    memcpy(&tab[(size_t)j * HERD_TAB_IN], &tpts[(size_t)j * 16], 64);
    tab[(size_t)j * HERD_TAB_IN + 16] = (u32)s[j].lo, tab[(size_t)j * HERD_TAB_IN + 17] = (u32)(s[j].lo >> 32);
    tab[(size_t)j * HERD_TAB_IN + 18] = (u32)s[j].hi, tab[(size_t)j * HERD_TAB_IN + 19] = (u32)(s[j].hi >> 32);
  }
  HIPCHK(h, hipMemcpyAsync(h->d_herdtab.p, tab.data(), tab.size() * sizeof(u32), hipMemcpyHostToDevice, h->stream));
  // the starts, a chunk of kangaroos at a time: (B + r_i) G and r_i G by the double-and-add kernel, then Q added to the wild ones
  herd_q q;
  memcpy(q.w, p.q, sizeof q.w);
  for (u32 first = 0; first < H; first += chunk) {
    const u32 n = H - first < chunk ? H - first : chunk;
    for (u32 t = 0; t < n; ++t) {
      const kg_u128 r = kg_offset(&st, p.sb);
      const uint64_t w[4] = {r.lo, r.hi, 0, 0};
      const u256 rv = u256_from(w);
      words_of(&ks[(size_t)t * 8], ((first + t) & 1u) ? rv : sc_add(p.base, rv));
      rs[(size_t)t * 4] = (u32)r.lo, rs[(size_t)t * 4 + 1] = (u32)(r.lo >> 32), rs[(size_t)t * 4 + 2] = (u32)r.hi, rs[(size_t)t * 4 + 3] = (u32)(r.hi >> 32);
    }
    HIPCHK(h, hipMemcpyAsync(d_k.p, ks.data(), (size_t)n * 8 * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_r.p, rs.data(), (size_t)n * 4 * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_mul_g, dim3((n + 63) / 64), dim3(64), 0, h->stream, d_k.p, d_pts.p, d_ok.p, n);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_herd_init, dim3((n + 63) / 64), dim3(64), 0, h->stream, d_pts.p, d_ok.p, d_r.p, q, h->d_herd.p, H, first, n, h->d_counter.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));  // the host buffers are filled again
  }
  HIPCHK(h, hipMemcpy(flags, h->d_counter.p + CW_HERD_FLAGS, sizeof(u32), hipMemcpyDeviceToHost));
  return ECL_OK;
}

// ecl_hip_add_range of a herd context: nkeys jumps, nkeys / H per kangaroo
static int herd_add_core(ecl_hip* h, const uint64_t blk[16], uint64_t nkeys, ecl_found* out, uint32_t cap, uint32_t* nout) {
  *nout = 0;
  herd_params p;
  int rc;
  if ((rc = herd_parse(h, blk, p)) != ECL_OK) return rc;
  const u32 H = 1u << p.herd_log2;
  if (nkeys % H) {
    h->err = "nkeys is not a multiple of the herd";
    return ECL_E_ARG;
  }
  call_frame f = {h, "add_range", nullptr, nkeys, out, cap, nout, false, true};
  if ((rc = f.begin()) != ECL_OK) return rc;
  const u32 L = (H + HERD_M - 1) / HERD_M, grid = (L + HERD_BLOCK - 1) / HERD_BLOCK, T = grid * HERD_BLOCK;
  if ((rc = ensure_scratch(h, (size_t)T * HERD_M * 2)) != ECL_OK) return rc;
  if ((rc = f.reset()) != ECL_OK) return rc;
  const bool cont = h->herd_valid && memcmp(h->herd_blk, blk, sizeof h->herd_blk) == 0;
  if (!cont) {
    h->herd_valid = false;
    u32 flags = 0;
    HIPCHK(h, hipEventRecord(h->ev_s0, h->stream));
    if ((rc = herd_build(h, p, &flags)) != ECL_OK) return rc;
    HIPCHK(h, hipEventRecord(h->ev_s1, h->stream));
    if (flags & HERD_FLAG_INFINITY) {
      h->err = "a kangaroo's start is the point at infinity";
      return ECL_E_RANGE;
    }
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));  // the walk's time starts behind the set-up
  }
  const add_args c = f.args();  // (no filter: the records, the counters, the jumps counted where the keys are)
  herd_args a;
  a.tab = h->d_herdtab.p, a.state = h->d_herd.p, a.scratch = h->d_scr.p, a.scratch2 = h->d_scr2.p;
  a.found = (uint4*)c.found, a.counter = c.counter, a.jumps = c.keys, a.cap = c.cap;
  a.H = H, a.L = L, a.T = T, a.dpmask = h->offs >= 32 ? ~0u : (1u << h->offs) - 1u;
  u64 per = (1ull << HERD_LAUNCH_JUMPS_LOG2) >> p.herd_log2;
  if (per > HERD_LAUNCH_STEPS_MAX) per = HERD_LAUNCH_STEPS_MAX;
  for (u64 left = nkeys / H; left;) {
    const u64 n = left < per ? left : per;
    a.steps = (u32)n;
    if (h->diag_drop) h->diag_drop = false, a.steps -= 1;  // (test hook: every kangaroo makes one jump fewer, so the count falls short)
    hipLaunchKernelGGL(k_herd_walk, dim3(grid), dim3(HERD_BLOCK), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    left -= n;
  }
  if ((rc = f.collect()) != ECL_OK) return rc;
  rc = f.finish(1, cont ? 0 : 1);
  h->herd_valid = false;
  if (rc == ECL_E_COVERAGE) return rc;  // the herd is not where the caller thinks it is: built anew next time
  if (herd_flags(h->pin_counter.p) & HERD_FLAG_DISTANCE) return f.refuse(ECL_E_RANGE, "a kangaroo's distance passed 2^128");
  h->herd_valid = true;
  memcpy(h->herd_blk, blk, sizeof h->herd_blk);
  return rc;
}
