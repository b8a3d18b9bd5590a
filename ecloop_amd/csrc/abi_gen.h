// abi_gen.h - host side of ecl_hip_mul_batch_raw on an ECL_GEN context: the template (host/gen_plan.h) is checked, kept and uploaded
// when it changes; k_gen_lines (gen.h) writes every piece's candidates and line table in front of the piece's hashing, on the stream the
// hashing runs on.  (one translation unit: included by ecloop_hip.hip after abi_mul.h)
#pragma once

// the kernel's view of an accepted template
// (arguments, slot size and table size: gen.h's, shared with the host harness)
static gen_args gen_args_of(const gen_info& gi) { return gen_args_make(gi.npos, gi.alt_at, gi.pool_at, gi.count, gi.first); }
static u32 gen_stride_of(const gen_info& gi) { return gen_stride_bytes(gi.L); }
static std::vector<u32> gen_image(const uint8_t* blob, size_t bytes) {
  std::vector<u32> img(gen_table_words(bytes), 0u);
  memcpy(img.data(), blob, bytes);
  return img;
}
// one k_gen_lines launch (the call's and the self-test's)
static void gen_launch(hipStream_t st, const u32* d_tab, const gen_args& g, u64 first, u32 m, u32 stride, u32 text_at, u32* d_text, u64* d_lines) {
  const u32 threads = (m + GEN_R - 1u) / GEN_R;
  hipLaunchKernelGGL(k_gen_lines, dim3((threads + 255u) / 256u), dim3(256), 0, st, d_tab, g, first, m, stride, text_at, d_text, d_lines);
}

// the body of ecl_hip_mul_batch_raw on such a context; the arguments have passed that function's checks and n >= 1.  blob: the template;
// lines[0]: the index of the call's first candidate
static int gen_batch(ecl_hip* h, const uint8_t* blob, uint32_t blob_bytes, const uint64_t* lines, uint32_t n, ecl_found* out, uint32_t cap, uint32_t* nout) {
  gen_info gi;
  if (const char* why = gen_blob_check(blob, blob_bytes, &gi)) {
    h->err = std::string("mul_batch_raw (gen): ") + why;
    return ECL_E_ARG;
  }
  const u64 first = lines[0];
  if (first > gi.T || n > gi.T - first) {
    h->err = "mul_batch_raw (gen): first + n passes the template's number of candidates";
    return ECL_E_ARG;
  }
  call_frame f = {h, "mul_batch_raw", (h->flags & ECL_TR) ? "mul_batch_raw" : nullptr, n, out, cap, nout, true, false};
  int rc;
  if ((rc = f.begin()) != ECL_OK) return rc;
  u32 W;
  if ((rc = mul_setup_auto(h, n, &W)) != ECL_OK) return rc;
  const wtab gtab = wtab_make(h->d_multab, W);
  h->mul_seen += n;
  // The device text is MUL_NBUF regions, one per staging buffer, of one slot per candidate of the largest piece.  A piece is at most the
  // staging buffer, the call, or one and a half pieces of twelve scalars per resident thread (mul_pieces: the merged last piece) - with
  // 256-byte slots the regions of that stay below 2^32 bytes; a piece that did not fit its region would be refused before its launch.
  const u32 stride = gen_stride_of(gi);
  u64 piece_cap = h->kbuf_cap < n ? h->kbuf_cap : n;
  if (piece_cap > (u64)MUL_NT * 18u) piece_cap = (u64)MUL_NT * 18u;
  const u64 region = piece_cap * stride, text_bytes64 = region * MUL_NBUF;
  if (text_bytes64 > 0xFFFFFFF0ull) {
    h->err = "mul_batch_raw (gen): the candidates of a piece do not fit the device text";
    return ECL_E_ARG;
  }
  const u32 text_bytes = (u32)text_bytes64;
  if ((rc = raw_buffers(h, text_bytes, n)) != ECL_OK) return rc;
  // the table: uploaded when it differs from the one the context holds (a host copy says so), behind every kernel that reads the old one
  const bool same = h->gen_blob.size() == blob_bytes && memcmp(h->gen_blob.data(), blob, blob_bytes) == 0 && h->d_gen.p;
  if (!same) {
    HIPCHK(h, hipStreamSynchronize(h->prep_stream));
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    h->gen_blob.clear();
    h->gen_img = gen_image(blob, blob_bytes);
    if (h->gen_img.size() > h->d_gen.n) {
      size_t capw = 1u << 10;
      while (capw < h->gen_img.size()) capw <<= 1;
      HIPCHK(h, h->d_gen.grow(capw));
    }
    HIPCHK(h, hipMemcpyAsync(h->d_gen.p, h->gen_img.data(), h->gen_img.size() * sizeof(u32), hipMemcpyHostToDevice, h->copy_stream));  // (in front of ev_copied[0])
    h->gen_blob.assign(blob, blob + blob_bytes);
  }
  const gen_args g = gen_args_of(gi);
  u64* d_lines = h->d_rawlines.p;
  u32* d_flags = h->d_counter.p + CW_RAW_OUTSIDE;
  u32* d_text = h->d_rawtext.p;
  const u32* d_tab = h->d_gen.p;
  if ((rc = f.reset()) != ECL_OK) return rc;
  HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));  // the hashing writes the flags: behind their reset
  HIPCHK(h, hipStreamWaitEvent(h->prep_stream, h->ev_fork, 0));
  rc = mul_pieces(
      h, n, gtab, f.args(), [](u32, u32, u32) -> int { return ECL_OK; },  // nothing to copy: the piece's first index is a kernel argument
      [&](u32 b, u32 at, u32 m, hipEvent_t* ready) -> int {
        if (m > piece_cap) {
          h->err = "mul_batch_raw (gen): a piece is larger than its region of the device text";
          return ECL_E_ARG;
        }
        // on the hashing's stream, which is in order: region b is written again only behind the hash of the piece that used it last
        HIPCHK(h, hipStreamWaitEvent(h->prep_stream, h->ev_copied[b], 0));
        gen_launch(h->prep_stream, d_tab, g, first + at, m, stride, (u32)(region * b), d_text, d_lines + at);
        raw_scalars_launch(h->kdf, h->prep_stream, d_text, text_bytes, text_bytes, d_lines + at, m, h->d_kbuf[b].p, d_flags);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipEventRecord(h->ev_hashed[b], h->prep_stream));
        *ready = h->ev_hashed[b];
        return ECL_OK;
      });
  if (rc != ECL_OK || (rc = f.collect()) != ECL_OK) return rc;
  if (raw_line_outside(h->pin_counter.p) || raw_line_late(h->pin_counter.p)) return f.refuse(ECL_E_SELFTEST, "mul_batch_raw (gen): a generated line lies outside the device text");
  return count_call(h, n, f.finish());
}

// a context with ECL_GEN: k_gen_lines, through the launch the call makes, on a built-in template against literal strings.  Four
// positions - {"ab", "c"}, {"", "xyz"}, {"-"}, {"0", "1", "2"}: words of three lengths, an empty one, a literal - and the candidates
// 3 ... 11: from 5 to 6 the last, the radix-1 and the second position all carry into the first, inside one thread's run; 3 is no multiple
// of GEN_R
static int gen_selftest(ecl_hip* h) {
  static const char* const WANT[9] = {"abxyz-0", "abxyz-1", "abxyz-2", "c-0", "c-1", "c-2", "cxyz-0", "cxyz-1", "cxyz-2"};
  gen_build b;
  memset(&b, 0, sizeof b);
  static const char* const ALTS[4][3] = {{"ab", "c", nullptr}, {"", "xyz", nullptr}, {"-", nullptr, nullptr}, {"0", "1", "2"}};
  for (int p = 0; p < 4; ++p) {
    gen_build_pos(&b);
    for (int a = 0; a < 3 && ALTS[p][a]; ++a) gen_build_alt(&b, (const uint8_t*)ALTS[p][a], strlen(ALTS[p][a]));
  }
  size_t bytes = 0;
  uint8_t* blob = gen_build_blob(&b, &bytes);
  gen_build_free(&b);
  gen_info gi;
  const char* why = blob ? gen_blob_check(blob, bytes, &gi) : "out of memory";
  std::vector<u32> img;
  if (!why) img = gen_image(blob, bytes);
  free(blob);
  if (why || gi.T != 12 || gi.L != 7) {
    h->err = "self-test of the candidate generator (ECL_GEN): the built-in template was refused";
    return ECL_E_SELFTEST;
  }
  const u32 m = 9, stride = gen_stride_of(gi), text_at = 2 * stride;  // (the region starts behind two untouched slots)
  const u32 text_words = (text_at + m * stride) / 4u + 2u;
  devbuf<u32> dtab, dtext;
  devbuf<u64> dlines;
  HIPCHK(h, hipSetDevice(h->dev));
  HIPCHK(h, dtab.grow(img.size()));
  HIPCHK(h, dtext.grow(text_words));
  HIPCHK(h, dlines.grow(m));
  HIPCHK(h, hipMemcpy(dtab.p, img.data(), img.size() * sizeof(u32), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemsetAsync(dtext.p, 0, text_words * sizeof(u32), h->stream));
  gen_launch(h->stream, dtab.p, gen_args_of(gi), 3, m, stride, text_at, dtext.p, dlines.p);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::vector<u32> text(text_words);
  u64 lines[9];
  HIPCHK(h, hipMemcpy(text.data(), dtext.p, text_words * sizeof(u32), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(lines, dlines.p, sizeof lines, hipMemcpyDeviceToHost));
  bool good = text[0] == 0 && text[text_at / 4u - 1u] == 0 && text[text_words - 2] == 0 && text[text_words - 1] == 0;
  for (u32 j = 0; j < m && good; ++j) {
    const u32 at = (u32)lines[j], len = (u32)(lines[j] >> 32);
    good = at == text_at + j * stride && len == strlen(WANT[j]) && memcmp((const char*)text.data() + at, WANT[j], len) == 0;
  }
  if (!good) {
    h->err = "self-test of the candidate generator (ECL_GEN) failed: k_gen_lines disagrees with the built-in template's candidates";
    return ECL_E_SELFTEST;
  }
  return ECL_OK;
}
