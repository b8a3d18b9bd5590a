// abi_seed.h - host side of ecl_hip_mul_batch_raw on an ECL_KDF_BIP39 context: the derivation record, the master stage over the whole
// call, the path stage in front of every `mul` piece.  (one translation unit: included by ecloop_hip.hip after abi_mul.h)
#pragma once

#define SEED_MAX_PHRASES (1u << 22)
#define SEED_MASTER_LAUNCH (1u << 20)  /* phrases of one k_bip39_master launch */

// lines[0] of a call: u8 magic[4] = "B39\0", reuse, depth, pass_len, zero; u32 path[depth]; u8 pass[pass_len] - packed, little-endian
struct seed_record {
  bool reuse;
  bip32_path path;
  u32 pass_len;
  uint8_t pass[BIP39_PASS_MAX];
};
// nullptr, or why the record is refused
static const char* seed_parse_record(seed_record* r, const uint8_t* p, u32 len) {
  if (len < 8u) return "mul_batch_raw (bip39): the derivation record is shorter than its header";
  if (memcmp(p, "B39\0", 4) != 0) return "mul_batch_raw (bip39): the first line is not a derivation record (magic \"B39\\0\")";
  const u32 reuse = p[4], depth = p[5], pass_len = p[6];
  if (depth > BIP32_DEPTH_MAX) return "mul_batch_raw (bip39): a path has at most 10 elements";
  if (pass_len > BIP39_PASS_MAX) return "mul_batch_raw (bip39): a passphrase has at most 99 bytes";
  if (reuse > 1u || p[7] != 0) return "mul_batch_raw (bip39): the record's reuse byte is 0 or 1 and its last header byte 0";
  if (len != 8u + 4u * depth + pass_len) return "mul_batch_raw (bip39): the record's length is not 8 + 4 * depth + pass_len";
  memset(r, 0, sizeof *r);
  r->reuse = reuse != 0, r->path.depth = depth, r->pass_len = pass_len;
  memcpy(r->path.el, p + 8, 4 * (size_t)depth);
  memcpy(r->pass, p + 8 + 4 * (size_t)depth, pass_len);
  return nullptr;
}

// one k_bip39_master / k_bip32_path launch (the call's and the self-test's)
static void seed_master_launch(hipStream_t st, const u32* d_text, u32 text_bytes, const u64* d_lines, u32 m, const bip39_salt& salt, u32* d_nodes) {
  hipLaunchKernelGGL(k_bip39_master, dim3((m + 63) / 64), dim3(64), 0, st, d_text, text_bytes, d_lines, m, salt, d_nodes);
}
static void seed_path_launch(hipStream_t st, const u32* d_nodes, u32 m, const bip32_path& path, const u32* d_gtab, u32* d_out) {
  hipLaunchKernelGGL(k_bip32_path, dim3((m + 63) / 64), dim3(64), 0, st, d_nodes, m, path, d_gtab, d_out);
}

// the body of ecl_hip_mul_batch_raw on such a context; the arguments have passed that function's checks and n >= 1
static int seed_batch(ecl_hip* h, const uint8_t* text, uint32_t text_bytes, const uint64_t* lines, uint32_t n, ecl_found* out, uint32_t cap, uint32_t* nout) {
  const bool last_ok = h->seed_last_ok;
  h->seed_last_ok = false;  // until this call has returned ECL_OK or ECL_E_OVERFLOW
  seed_record rec;
  {
    const u64 r0 = lines[0], at = r0 & 0xFFFFFFFFull, len = r0 >> 32;
    if (at + len > text_bytes) {
      h->err = "mul_batch_raw (bip39): the derivation record lies outside the text";
      return ECL_E_ARG;
    }
    if (const char* why = seed_parse_record(&rec, text + at, (u32)len)) {
      h->err = why;
      return ECL_E_ARG;
    }
  }
  const u32 np = n - 1;  // phrases: lines[1 .. n - 1]
  if (np > SEED_MAX_PHRASES) {
    h->err = "mul_batch_raw (bip39): more than 2^22 phrases in one call";
    return ECL_E_ARG;
  }
  if (rec.reuse) {
    const char* why = !h->seed_have ? "mul_batch_raw (bip39): reuse = 1, but the context keeps no nodes"
                      : !last_ok ? "mul_batch_raw (bip39): reuse = 1 after a call that did not succeed"
                      : np != h->seed_n ? "mul_batch_raw (bip39): reuse = 1 with another number of phrases than the call before"
                      : rec.pass_len != h->seed_pass_len || memcmp(rec.pass, h->seed_pass, rec.pass_len) != 0
                          ? "mul_batch_raw (bip39): reuse = 1 with another passphrase than the kept nodes'"
                          : nullptr;
    if (why) {
      h->err = why;
      return ECL_E_ARG;
    }
  } else {
    h->seed_have = false;
    for (u32 i = 1; i < n; ++i)
      if ((lines[i] & 0xFFFFFFFFull) + (lines[i] >> 32) > text_bytes) {
        h->err = "mul_batch_raw: a line of the table lies outside the text";
        return ECL_E_ARG;
      }
  }
  if (np == 0) {  // the record alone: nothing to derive
    if (!rec.reuse) h->seed_have = true, h->seed_n = 0, h->seed_pass_len = rec.pass_len, memcpy(h->seed_pass, rec.pass, sizeof rec.pass);
    h->last.forget();
    h->seed_last_ok = true;
    return ECL_OK;
  }
  call_frame f = {h, "mul_batch_raw", (h->flags & ECL_TR) ? "mul_batch_raw" : nullptr, np, out, cap, nout, true, false};
  int rc;
  if ((rc = f.begin()) != ECL_OK) return rc;
  u32 W;
  if ((rc = mul_setup_auto(h, np, &W)) != ECL_OK) return rc;
  if ((rc = ensure_gtable(h)) != ECL_OK) return rc;
  const wtab gtab = wtab_make(h->d_multab, W);
  h->mul_seen += np;
  if ((rc = raw_buffers(h, rec.reuse ? 0 : text_bytes, rec.reuse ? 0 : n)) != ECL_OK) return rc;
  if ((size_t)np * BIP39_NODE_WORDS > h->d_nodes.n) {  // (only a reuse = 0 call gets here with too small a buffer)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->prep_stream));
    u32 capn = 1u << 10;
    while (capn < np) capn <<= 1;
    HIPCHK(h, h->d_nodes.grow((size_t)capn * BIP39_NODE_WORDS));
  }
  if ((rc = f.reset()) != ECL_OK) return rc;
  if (!rec.reuse) {
    // The master stage for the whole call up front, the text and the table sent first: a `mul` piece of 2^16 lines is one wave per SIMD
    // for a kernel that runs tens of milliseconds per lane, so it cannot fill the chip piece by piece.
    bip39_salt salt;
    bip39_salt_block(salt, rec.pass, rec.pass_len);
    HIPCHK(h, hipMemcpyAsync(h->d_rawtext.p, text, text_bytes, hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(h, hipMemcpyAsync(h->d_rawlines.p, lines, (size_t)n * 8, hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(h, hipEventRecord(h->ev_copied[0], h->copy_stream));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_copied[0], 0));
    for (u32 at = 0; at < np; at += SEED_MASTER_LAUNCH) {
      const u32 m = np - at < SEED_MASTER_LAUNCH ? np - at : SEED_MASTER_LAUNCH;
      seed_master_launch(h->stream, h->d_rawtext.p, text_bytes, h->d_rawlines.p + 1 + at, m, salt, h->d_nodes.p + (size_t)at * BIP39_NODE_WORDS);
      HIPCHK(h, hipGetLastError());
    }
    h->seed_n = np, h->seed_pass_len = rec.pass_len;
    memcpy(h->seed_pass, rec.pass, sizeof rec.pass);
  }
  HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));  // the path stage reads the nodes: behind the master stage (and the counters' reset)
  HIPCHK(h, hipStreamWaitEvent(h->prep_stream, h->ev_fork, 0));
  const u32* d_nodes = h->d_nodes.p;
  const u32* d_gtab = h->d_gtab.p;
  rc = mul_pieces(
      h, np, gtab, f.args(), [](u32, u32, u32) -> int { return ECL_OK; },
      [&](u32 b, u32 at, u32 m, hipEvent_t* ready) -> int {  // k_bip32_path where `mul -raw` hashes the piece's lines
        seed_path_launch(h->prep_stream, d_nodes + (size_t)at * BIP39_NODE_WORDS, m, rec.path, d_gtab, h->d_kbuf[b].p);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipEventRecord(h->ev_hashed[b], h->prep_stream));
        *ready = h->ev_hashed[b];
        return ECL_OK;
      });
  if (rc != ECL_OK || (rc = f.collect()) != ECL_OK) return rc;
  rc = count_call(h, np, f.finish());
  if (rc == ECL_OK || rc == ECL_E_OVERFLOW) h->seed_last_ok = true, h->seed_have = true;
  return rc;
}

// a context with ECL_KDF_BIP39: both kernels, through the launches the call makes, on BIP39's test phrase ("abandon" x 11 + "about", at
// a start that is not word-aligned): its master key without a passphrase and with "TREZOR", and its m/44'/0'/0'/0/0 key
static int seed_selftest(ecl_hip* h) {
  static const char TEXT[] = "xabandon abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon about";
  static const char* const WANT[2][2] = {
      {"1837c1be8e2995ec11cda2b066151be2cfb48adf9e47b151d46adab3a21cdf67", "e284129cc0922579a535bbf4d1a3b25773090d28c909bc0fed73b5e0222cc372"},
      {"cbedc75b0d6412c85c79bc13875112ef912fd1e756631b5a00330866f22ff184", nullptr}};
  const u32 text_bytes = sizeof TEXT - 1;
  const u64 line = 1ull | (u64)(text_bytes - 1) << 32;
  std::vector<u32> words((text_bytes + 3) / 4 + 2, 0u);
  memcpy(words.data(), TEXT, text_bytes);
  devbuf<u32> dtext, dnode, dout;
  devbuf<u64> dline;
  HIPCHK(h, hipSetDevice(h->dev));
  int rc;
  if ((rc = ensure_gtable(h)) != ECL_OK) return rc;
  HIPCHK(h, dtext.grow(words.size()));
  HIPCHK(h, dline.grow(1));
  HIPCHK(h, dnode.grow(BIP39_NODE_WORDS));
  HIPCHK(h, dout.grow(16));
  HIPCHK(h, hipMemcpy(dtext.p, words.data(), words.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(dline.p, &line, 8, hipMemcpyHostToDevice));
  bool good = true;
  for (int t = 0; t < 2 && good; ++t) {
    bip39_salt salt;
    bip39_salt_block(salt, (const uint8_t*)"TREZOR", t ? 6u : 0u);
    bip32_path p0 = {}, p44 = {5, {44u | 1u << 31, 1u << 31, 1u << 31, 0, 0}};
    seed_master_launch(h->stream, dtext.p, text_bytes, dline.p, 1, salt, dnode.p);
    seed_path_launch(h->stream, dnode.p, 1, p0, h->d_gtab.p, dout.p);
    seed_path_launch(h->stream, dnode.p, 1, p44, h->d_gtab.p, dout.p + 8);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    u32 got[16];
    HIPCHK(h, hipMemcpy(got, dout.p, sizeof got, hipMemcpyDeviceToHost));
    for (int i = 0; i < 2 && good; ++i) {
      if (!WANT[t][i]) continue;
      char hex[65];
      for (int w = 0; w < 8; ++w) snprintf(hex + 8 * w, 9, "%08x", got[i * 8 + 7 - w]);
      good = memcmp(hex, WANT[t][i], 64) == 0;
    }
  }
  if (!good) {
    h->err = "known-answer test of the BIP39 / BIP32 derivation (ECL_KDF_BIP39) failed";
    return ECL_E_SELFTEST;
  }
  return ECL_OK;
}
