// abi_tr.h - host side of the Taproot search (ECL_TR): `add` walked in slabs (emit, then k_tr_check), the piece of `mul`, ecl_hip_verify_tr,
// ecl_hip_diag_tr.  (one translation unit: included by ecloop_hip.hip after abi_mul.h)
#pragma once

// keys per slab of a Taproot `add` call: 2^26 (6.4 GB of t and P'), a multiple of the sweep of the geometry such a launch takes, so that
// the resident walk runs on from slab to slab; ECL_HIP_TR_SLAB_LOG2 = 12 ... 28 for tests and tuning - it changes no result
#define TR_SLAB_LOG2_DEFAULT 26u
static u64 tr_slab_keys() {
  const char* e = getenv("ECL_HIP_TR_SLAB_LOG2");
  long v = e && e[0] ? strtol(e, nullptr, 10) : (long)TR_SLAB_LOG2_DEFAULT;
  if (v < 12 || v > 28) v = TR_SLAB_LOG2_DEFAULT;
  return 1ull << v;
}
// stage B walks a slab in launches of TR_CHUNK entries - what the chip holds at once at TR_R keys per thread, the size of `mul`'s full
// pieces - alternating between the context's two compute streams, each with its own parking space, as `mul`'s pieces do
#define TR_CHUNK (MUL_NT * TR_R)
static void tr_geometry(u32 m, u32* R, u32* nt) { mul_geometry(m, TR_R, R, nt); }  // (m > TR_CHUNK - a long piece of `mul`: more threads than are resident)
static u64 tr_tmp_words(u64 m) {
  u32 R, nt;
  tr_geometry((u32)(m < TR_CHUNK ? m : TR_CHUNK), &R, &nt);
  return (u64)R * nt * 27u;
}
// the `mul` table of a Taproot `add` call of nkeys keys: the width policy and accounting of `mul` - tweaked keys are scalars seen
static int tr_table(ecl_hip* h, u64 nkeys, wtab* gtab) {
  u32 W;
  const int rc = mul_at_width_in_force(h, nkeys, &W, [&](u32 w) { return ensure_multable(h, w); });
  if (rc == ECL_OK) *gtab = wtab_make(h->d_multab, W);
  return rc;
}
static int tr_buffers(ecl_hip* h, u64 nkeys) {
  const u64 slab = tr_slab_keys(), m = nkeys < slab ? nkeys : slab, words = tr_tmp_words(m);
  int rc;
  if ((rc = mul_streams(h)) != ECL_OK) return rc;
  if (h->d_trslab.n < m * TR_SLAB_WORDS) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream2));
    HIPCHK(h, h->d_trslab.grow((size_t)m * TR_SLAB_WORDS));
  }
  if (held_by_all(h->d_trtmp) < words) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream2));
    for (int i = 0; i < 2; ++i) HIPCHK(h, h->d_trtmp[i].grow((size_t)words));
  }
  return ECL_OK;
}
static int tr_reserve(ecl_hip* h, uint64_t nkeys) {
  int rc;
  wtab gtab;
  if ((rc = tr_table(h, nkeys, &gtab)) != ECL_OK) return rc;
  if ((rc = tr_buffers(h, nkeys)) != ECL_OK) return rc;
  const u64 slab = tr_slab_keys(), m = nkeys < slab ? nkeys : slab;
  if (!nkeys_ok(h, m)) return ECL_E_ARG;
  u32 B, nb, T;
  call_geometry(h, m, B, nb, T);
  return ensure_walk_buffers(h, B, T);
}
// stage B over `m` entries of `slab` (m <= TR_CHUNK) on stream `st`: records with key_offset = base + entry index, counted where `a` says
// (the frame's args(CW_TR_CHECKED))
static int tr_launch_check(ecl_hip* h, hipStream_t st, const u32* slab, u32 m, u64 base, const wtab& gtab, const add_args& a, u32 epoch, u32* tmp) {
  u32 R, nt;
  tr_geometry(m, &R, &nt);
  hipLaunchKernelGGL(k_tr_check<false>, dim3(nt / 256), dim3(256), 0, st, slab, m, base, gtab, a, epoch, tmp, nt, R, (u32*)nullptr, (u8*)nullptr);
  HIPCHK(h, hipGetLastError());
  return ECL_OK;
}
// ... over a whole slab of the `add` path, which the emit kernel has just been queued for on h->stream: the second stream joins in behind
// it, and h->stream goes on (the next slab's emit kernel, the read-back) when both are done
static int tr_check_slab(ecl_hip* h, u64 m, u64 at, const wtab& gtab, const add_args& a, u32 epoch) {
  const bool two = m > TR_CHUNK;
  if (two) {
    HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
  }
  const u64 chunks = (m + TR_CHUNK - 1) / TR_CHUNK, even = ((m + chunks - 1) / chunks + 255u) / 256u * 256u;  // equal launches: no crumb at the end
  u32 c = 0;
  for (u64 off = 0; off < m; ++c) {
    const u64 n = m - off < even ? m - off : even;
    const int lane = two ? (int)(c & 1u) : 0;
    int rc = tr_launch_check(h, lane ? h->stream2 : h->stream, h->d_trslab.p + (size_t)off * TR_SLAB_WORDS, (u32)n, at + off, gtab, a, epoch, h->d_trtmp[lane].p);
    if (rc != ECL_OK) return rc;
    off += n;
  }
  if (two) {
    HIPCHK(h, hipEventRecord(h->ev_join, h->stream2));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));
  }
  return ECL_OK;
}

// ecl_hip_add_range's body on a Taproot context.  A call of 2^32 keys cannot park 2^32 x 96 bytes, so it is walked in slabs of contiguous
// sub-launches of the emit kernel (the points come from the walk), each followed by k_tr_check over the slab, all on the context's
// stream.  A slab that is a whole number of sweeps of its geometry (the default) hands the resident walk to the next one; any other
// re-positions.  The records of all slabs go to the call's one record buffer with key_offset counted from the call's start, so cap,
// ECL_E_OVERFLOW, ecl_hip_fetch_found, list mode and the look-ahead see one call.  The call is whole if the points emitted AND the
// entries that reached the probe step both equal nkeys.
static int tr_add_core(ecl_hip* h, const u256& k0, uint64_t nkeys, ecl_found* out, uint32_t cap, uint32_t* nout) {
  call_frame f = {h, "add_range (Taproot, points emitted)", "add_range (Taproot, output keys)", nkeys, out, cap, nout, false, false};
  int rc;
  if ((rc = f.begin()) != ECL_OK) return rc;
  wtab gtab;
  if ((rc = tr_table(h, nkeys, &gtab)) != ECL_OK) return rc;
  if ((rc = tr_buffers(h, nkeys)) != ECL_OK) return rc;
  h->mul_seen += nkeys;
  const u64 slab = tr_slab_keys();
  const u256 s = sc_pow2(h->offs);
  if ((rc = f.reset()) != ECL_OK) return rc;
  const add_args check = f.args(CW_TR_CHECKED);
  u32 slabs = 0, setups = 0;
  for (u64 at = 0; at < nkeys; ++slabs) {
    const u64 m = nkeys - at < slab ? nkeys - at : slab;
    h->tr_epoch ^= 1u;
    const add_launched l = add_launch(h, f, sc_add(k0, sc_mul_u64(s, at)), m, h->d_trslab.p);
    if (l.rc != ECL_OK) {
      h->walk_valid = false;
      return l.rc;
    }
    setups += l.continued ? 0u : 1u;
    if ((rc = tr_check_slab(h, m, at, gtab, check, h->tr_epoch)) != ECL_OK) return rc;
    at += m;
  }
  if ((rc = f.collect()) != ECL_OK) return rc;
  return f.finish(slabs, setups);  // (both stages of every slab; a call re-positions once, or at every odd slab for about as long each)
}

// a piece of `mul` on a Taproot context: the window sums' points into the piece's own slab (k_mul_points_tr), then k_tr_check over it, on
// the piece's stream; the two kernels share the stream's parking space
static void tr_mul_launch_piece(ecl_hip* h, int lane, const u32* d_k, u32 m, u32 at, const wtab& gtab, const add_args& a, bool short_round) {
  u32 R, nt;
  hipStream_t st = lane ? h->stream2 : h->stream;
  mul_geometry(m, MUL_R, &R, &nt);
  if (short_round) R -= 1;
  const u32 epoch = h->tr_epoch_mul[lane] ^= 1u;
  add_args e = a, check = a;
  e.slab = h->d_trslab_mul[lane].p, e.epoch = epoch;
  check.keys = (unsigned long long*)(a.counter + CW_TR_CHECKED);
  hipLaunchKernelGGL(k_mul_points_tr, dim3(nt / 256), dim3(256), 0, st, d_k, m, 0u, gtab, e, h->d_multmp[lane].p, nt, R);
  if (hipGetLastError() != hipSuccess) return;
  (void)tr_launch_check(h, st, h->d_trslab_mul[lane].p, m, at, gtab, check, epoch, h->d_multmp[lane].p);
}

extern "C" int ecl_hip_verify_tr(ecl_hip* h, const uint64_t (*k)[4], uint32_t n, uint32_t (*qx)[8], uint8_t* ok) {
  if (!h || !k || !qx || !ok || n == 0 || n > (1u << 31)) return ECL_E_ARG;
  HIPCHK(h, hipSetDevice(h->dev));
  int rc;
  if ((rc = ensure_gtable(h)) != ECL_OK) return rc;
  devbuf<u8> d;  // scalars 32 B, output key 32 B, flag
  HIPCHK(h, d.grow((size_t)n * 65));
  u32* dk = (u32*)d.p;
  u32* dq = (u32*)(d.p + (size_t)n * 32);
  u8* dok = d.p + (size_t)n * 64;
  HIPCHK(h, hipMemcpyAsync(dk, k, (size_t)n * 32, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_verify_tr, dim3((n + 63) / 64), dim3(64), 0, h->stream, dk, n, h->d_gtab.p, dq, dok);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(qx, dq, (size_t)n * 32, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(ok, dok, n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return ECL_OK;
}

// stage A (tr_emit) and stage B (k_tr_check) of the search path for n affine points: t[i] = the tweak of x[i], qx[i] = the output key,
// ok[i] = 0 where there is none.  No filter is involved; the context's coverage totals are left alone.
extern "C" int ecl_hip_diag_tr(ecl_hip* h, const uint64_t (*x)[4], const uint64_t (*y)[4], uint64_t (*t)[4], uint32_t (*qx)[8], uint8_t* ok, uint32_t n) {
  if (!h || !x || !y || !t || !qx || !ok || n == 0 || n > (1u << 20)) return ECL_E_ARG;
  HIPCHK(h, hipSetDevice(h->dev));
  int rc;
  wtab gtab;
  if ((rc = tr_table(h, 0, &gtab)) != ECL_OK) return rc;
  u32 R, nt;
  tr_geometry(n, &R, &nt);
  devbuf<u32> dx, dy, slab, tmp, dq;
  devbuf<u8> dok;
  devbuf<unsigned long long> cnt;
  HIPCHK(h, dx.grow((size_t)n * 8));
  HIPCHK(h, dy.grow((size_t)n * 8));
  HIPCHK(h, slab.grow((size_t)n * TR_SLAB_WORDS));
  HIPCHK(h, tmp.grow((size_t)R * nt * 27));
  HIPCHK(h, dq.grow((size_t)n * 8));
  HIPCHK(h, dok.grow(n));
  HIPCHK(h, cnt.grow(1));
  HIPCHK(h, hipMemcpyAsync(dx.p, x, (size_t)n * 32, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(dy.p, y, (size_t)n * 32, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(cnt.p, 0, 8, h->stream));
  add_args a;
  memset(&a, 0, sizeof a);
  a.slab = slab.p, a.epoch = 1u, a.keys = cnt.p;
  hipLaunchKernelGGL(k_tr_emit_points, dim3((n + 63) / 64), dim3(64), 0, h->stream, dx.p, dy.p, n, a);
  HIPCHK(h, hipGetLastError());
  a.slab = nullptr, a.epoch = 0;
  hipLaunchKernelGGL(k_tr_check<true>, dim3(nt / 256), dim3(256), 0, h->stream, slab.p, n, (u64)0, gtab, a, 1u, tmp.p, nt, R, dq.p, dok.p);
  HIPCHK(h, hipGetLastError());
  std::vector<u32> sl((size_t)n * TR_SLAB_WORDS);
  HIPCHK(h, hipMemcpyAsync(sl.data(), slab.p, sl.size() * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(qx, dq.p, (size_t)n * 32, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(ok, dok.p, n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (u32 i = 0; i < n; ++i) memcpy(t[i], &sl[(size_t)i * TR_SLAB_WORDS], 32);
  return ECL_OK;
}
