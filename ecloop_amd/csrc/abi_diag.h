// abi_diag.h - host side of the diagnostics entry points, the bulk bloom insert and the self-test.
// (one translation unit: included by ecloop_hip.hip last)
#pragma once
// ------------------------------------------------------------------------------------------------ diagnostics (host)

extern "C" int ecl_hip_diag_fe(ecl_hip* h, int op, const uint64_t (*a)[4], const uint64_t (*b)[4], uint64_t (*r)[4],
                               uint32_t n) {
  if (!h || !a || !r || n == 0 || op < 0 || op > 11) return ECL_E_ARG;
  HIPCHK(h, hipSetDevice(h->dev));
  size_t bytes = (size_t)n * 32;
  devbuf<u32> da, db, dr;
  HIPCHK(h, da.grow((size_t)n * 8));
  HIPCHK(h, db.grow((size_t)n * 8));
  HIPCHK(h, dr.grow((size_t)n * 8));
  HIPCHK(h, hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice));  // little-endian u64 limbs == u32 word pairs
  HIPCHK(h, hipMemcpy(db.p, b ? b : a, bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_diag_fe, dim3((n + 63) / 64), dim3(64), 0, h->stream, op, da.p, db.p, dr.p, n);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(r, dr.p, bytes, hipMemcpyDeviceToHost));
  return ECL_OK;
}

extern "C" int ecl_hip_diag_limbs(ecl_hip* h, int op, const uint32_t (*in)[LIMB_IN][FE_LIMBS], uint32_t (*out)[LIMB_OUT][FE_LIMBS],
                                  uint32_t* flag, uint32_t n) {
  if (!h || !in || !out || !flag || n == 0 || op < 0 || op >= LIMB_OPS) return ECL_E_ARG;
  HIPCHK(h, hipSetDevice(h->dev));
  const size_t bin = (size_t)n * LIMB_IN * FE_LIMBS * 4, bout = (size_t)n * LIMB_OUT * FE_LIMBS * 4;
  devbuf<u32> di, dout, df;
  HIPCHK(h, di.grow(bin / 4));
  HIPCHK(h, dout.grow(bout / 4));
  HIPCHK(h, df.grow(n));
  HIPCHK(h, hipMemcpy(di.p, in, bin, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_diag_limbs, dim3((unsigned)(((u64)n + 63) / 64)), dim3(64), 0, h->stream, op, di.p, dout.p, df.p, n);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, dout.p, bout, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(flag, df.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return ECL_OK;
}

extern "C" int ecl_hip_diag_mulg(ecl_hip* h, const uint64_t (*k)[4], uint64_t (*x)[4], uint64_t (*y)[4], uint8_t* ok,
                                 uint32_t n) {
  if (!h || !k || !x || !y || n == 0) return ECL_E_ARG;
  HIPCHK(h, hipSetDevice(h->dev));
  devbuf<u32> dk, dout;
  devbuf<u8> dok;
  HIPCHK(h, dk.grow((size_t)n * 8));
  HIPCHK(h, dout.grow((size_t)n * 16));
  HIPCHK(h, dok.grow(n));
  HIPCHK(h, hipMemcpy(dk.p, k, (size_t)n * 32, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_mul_g, dim3((n + 63) / 64), dim3(64), 0, h->stream, dk.p, dout.p, dok.p, n);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::vector<u32> o((size_t)n * 16);
  std::vector<u8> okv(n);
  HIPCHK(h, hipMemcpy(o.data(), dout.p, (size_t)n * 64, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(okv.data(), dok.p, n, hipMemcpyDeviceToHost));
  for (u32 i = 0; i < n; ++i) {
    memcpy(x[i], &o[(size_t)i * 16], 32);
    memcpy(y[i], &o[(size_t)i * 16 + 8], 32);
    if (ok) ok[i] = okv[i];
  }
  return ECL_OK;
}

extern "C" int ecl_hip_diag_hash160(ecl_hip* h, const uint64_t (*x)[4], const uint64_t (*y)[4], uint32_t (*h33)[5],
                                    uint32_t (*h65)[5], uint32_t n) {
  if (!h || !x || !y || !h33 || !h65 || n == 0) return ECL_E_ARG;
  HIPCHK(h, hipSetDevice(h->dev));
  devbuf<u32> dx, dy, d33, d65;
  HIPCHK(h, dx.grow((size_t)n * 8));
  HIPCHK(h, dy.grow((size_t)n * 8));
  HIPCHK(h, d33.grow((size_t)n * 5));
  HIPCHK(h, d65.grow((size_t)n * 5));
  HIPCHK(h, hipMemcpy(dx.p, x, (size_t)n * 32, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(dy.p, y, (size_t)n * 32, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_diag_hash, dim3((n + 63) / 64), dim3(64), 0, h->stream, dx.p, dy.p, d33.p, d65.p, n);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(h33, d33.p, (size_t)n * 20, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(h65, d65.p, (size_t)n * 20, hipMemcpyDeviceToHost));
  return ECL_OK;
}

extern "C" int ecl_hip_bloom_insert(ecl_hip* h, const uint32_t (*h160)[5], uint64_t n) {
  if (!h || (!h160 && n) || (h->flags & (ECL_PREFIX | ECL_MASK))) return ECL_E_ARG;
  if (!h->d_bloom.p) return ECL_E_NOBLOOM;
  if (n == 0) return ECL_OK;
  la_leave(h), h->la_key_valid = false;  // the resident filter is no longer the one that was uploaded: no shared look-ahead on it
  HIPCHK(h, hipSetDevice(h->dev));
  const u64 chunk = 1ull << 24;  // 320 MB of hashes per upload
  devbuf<u32> dh;
  HIPCHK(h, dh.grow((size_t)(n < chunk ? n : chunk) * 5));
  for (u64 at = 0; at < n; at += chunk) {
    u64 m = n - at < chunk ? n - at : chunk;
    HIPCHK(h, hipMemcpy(dh.p, h160 + at, (size_t)m * 20, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_bloom_insert, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream,
                       bloom_make(h->d_bloom.p, h->bloom_words), h->d_bloom.p, dh.p, m);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return ECL_OK;
}

extern "C" int ecl_hip_bloom_insert_count(ecl_hip* h, const uint32_t (*h160)[5], uint64_t n, uint64_t* added) {
  if (!h || (!h160 && n) || !added || (h->flags & (ECL_PREFIX | ECL_MASK))) return ECL_E_ARG;
  *added = 0;
  if (!h->d_bloom.p) return ECL_E_NOBLOOM;
  if (n == 0) return ECL_OK;
  if (h->bloom_words >= (1ull << (64 - BLF_CHUNK_LOG2 - 6))) return ECL_E_ARG;  // bit position must fit 44 bits (2 TB filter)
  la_leave(h), h->la_key_valid = false;
  HIPCHK(h, hipSetDevice(h->dev));
  const u64 chunk = 1ull << BLF_CHUNK_LOG2;
  devbuf<u32> dh;
  devbuf<u64> tab;
  devbuf<unsigned long long> cnt;
  HIPCHK(h, dh.grow((size_t)(n < chunk ? n : chunk) * 5));
  HIPCHK(h, tab.grow((size_t)1 << BLF_TAB_LOG2));
  HIPCHK(h, cnt.grow(1));
  HIPCHK(h, hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), h->stream));
  const bloom_t b = bloom_make(h->d_bloom.p, h->bloom_words);
  for (u64 at = 0; at < n; at += chunk) {
    const u32 m = (u32)(n - at < chunk ? n - at : chunk);
    HIPCHK(h, hipMemcpyAsync(dh.p, h160 + at, (size_t)m * 20, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(tab.p, 0xFF, sizeof(u64) << BLF_TAB_LOG2, h->stream));
    hipLaunchKernelGGL(k_blf_claim, dim3((m + 255) / 256), dim3(256), 0, h->stream, b, dh.p, m, tab.p);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_blf_count_and_set, dim3((m + 255) / 256), dim3(256), 0, h->stream, b, h->d_bloom.p, dh.p, m, tab.p, cnt.p);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_bloom_insert, dim3((m + 255) / 256), dim3(256), 0, h->stream, b, h->d_bloom.p, dh.p, (u64)m);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));  // the host buffer slice is free again; next chunk sees these bits
  }
  unsigned long long c = 0;
  HIPCHK(h, hipMemcpy(&c, cnt.p, sizeof c, hipMemcpyDeviceToHost));
  *added = c;
  return ECL_OK;
}

extern "C" int ecl_hip_get_bloom(ecl_hip* h, uint64_t* bits, uint64_t nwords) {
  if (!h || !bits || (h->flags & (ECL_PREFIX | ECL_MASK))) return ECL_E_ARG;
  if (!h->d_bloom.p) return ECL_E_NOBLOOM;
  if (nwords != h->bloom_words) return ECL_E_ARG;
  HIPCHK(h, hipSetDevice(h->dev));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(bits, h->d_bloom.p, nwords * sizeof(u64), hipMemcpyDeviceToHost));
  return ECL_OK;
}

extern "C" int ecl_hip_diag_bloom(ecl_hip* h, const uint32_t (*h160)[5], uint8_t* hit, uint32_t n) {
  if (!h || !h160 || !hit || n == 0) return ECL_E_ARG;
  if (!h->d_bloom.p) return ECL_E_NOBLOOM;
  HIPCHK(h, hipSetDevice(h->dev));
  devbuf<u32> dh;
  devbuf<u8> dhit;
  HIPCHK(h, dh.grow((size_t)n * 5));
  HIPCHK(h, dhit.grow(n));
  HIPCHK(h, hipMemcpy(dh.p, h160, (size_t)n * 20, hipMemcpyHostToDevice));
  if (h->flags & ECL_PREFIX)  // the device's two-stage prefix test on the given values
    hipLaunchKernelGGL(k_diag_prefix, dim3((n + 63) / 64), dim3(64), 0, h->stream, prefix_of(h), dh.p, dhit.p, n);
  else if (h->flags & ECL_MASK)  // the device's mask test on the given values
    hipLaunchKernelGGL(k_diag_mask, dim3((n + 63) / 64), dim3(64), 0, h->stream, mask_of(h), dh.p, dhit.p, n);
  else
    hipLaunchKernelGGL(k_diag_bloom, dim3((n + 63) / 64), dim3(64), 0, h->stream, bloom_make(h->d_bloom.p, h->bloom_words),
                       dh.p, dhit.p, n);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(hit, dhit.p, n, hipMemcpyDeviceToHost));
  return ECL_OK;
}

extern "C" int ecl_hip_diag_bloom_mod(ecl_hip* h, uint64_t nwords, const uint64_t* x, uint64_t* r, uint32_t n) {
  if (!h || !x || !r || n == 0 || nwords == 0 || nwords >= (1ull << 58)) return ECL_E_ARG;
  HIPCHK(h, hipSetDevice(h->dev));
  devbuf<u64> dx, dr;
  HIPCHK(h, dx.grow(n));
  HIPCHK(h, dr.grow(n));
  HIPCHK(h, hipMemcpy(dx.p, x, (size_t)n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_diag_bloom_mod, dim3((n + 63) / 64), dim3(64), 0, h->stream, bloom_make(nullptr, nwords), dx.p, dr.p, n);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(r, dr.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return ECL_OK;
}

// test hook of the key-coverage check: the next search launch (add_range, a look-ahead sweep, or the first piece of a mul call) runs one
// round short - the add kernel one group per lane fewer, the mul kernel one scalar per thread fewer - so that keys of the call are not
// hashed and the call has to fail with ECL_E_COVERAGE.  Only a loop bound shrinks: the launch touches a part of what it touches anyway.
extern "C" int ecl_hip_diag_drop_round(ecl_hip* h) {
  if (!h) return ECL_E_ARG;
  h->diag_drop = true;
  return ECL_OK;
}

// ------------------------------------------------------------------------------------------------ self-test

// a context with ECL_KDF_* bits: its hashing kernel on known answers (computed elsewhere: FIPS 202's SHA3-256 vectors, Keccak-256 and the
// 2031-fold form from an independent implementation), through the launch ecl_hip_mul_batch_raw makes.  The three lines share one text:
// "" and "abc" at offset 0, "password" at offset 3 (a start that is not word-aligned).
static int kdf_selftest(ecl_hip* h) {
  static const char TEXT[] = "abcpassword";
  static const u64 LINES[3] = {0ull, 3ull << 32, 3ull | 8ull << 32};
  static const char* const KAT[3][3] = {
      {"c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470", "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45", nullptr},
      {"a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a", "3a985da74fe225b2045c172d6bd390bd855f086e3e9d525b46bfe24511431532", nullptr},
      {"26d412aa8b9fea49149a7dbf8b19672d8813f741842ac1847571d335908cbe65", "7a44789ed3cd85861c0bbf9693c7e1de1862dd4396c390147ecf1275099c6e6f",
       "5e225b381fcf02bd5577885f19b9472234c117dc44df6b59aca6690471dea0a0"}};
  const char* const* want = KAT[h->kdf == ECL_KDF_KECCAK ? 0 : h->kdf == ECL_KDF_SHA3 ? 1 : 2];
  const u32 text_bytes = sizeof TEXT - 1;
  u32 words[5] = {};  // three words of text and the two spare ones
  memcpy(words, TEXT, text_bytes);
  devbuf<u32> dtext, dout;
  devbuf<u64> dlines;
  HIPCHK(h, hipSetDevice(h->dev));
  HIPCHK(h, dtext.grow(5));
  HIPCHK(h, dlines.grow(3));
  HIPCHK(h, dout.grow(3 * 8 + 2));  // three scalars, then the two flags of the kernel
  HIPCHK(h, hipMemcpy(dtext.p, words, sizeof words, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(dlines.p, LINES, sizeof LINES, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemsetAsync(dout.p, 0, (3 * 8 + 2) * sizeof(u32), h->stream));
  raw_scalars_launch(h->kdf, h->stream, dtext.p, text_bytes, text_bytes, dlines.p, 3, dout.p, dout.p + 24);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  u32 got[3 * 8 + 2];
  HIPCHK(h, hipMemcpy(got, dout.p, sizeof got, hipMemcpyDeviceToHost));
  bool good = got[24] == 0 && got[25] == 0;
  for (int i = 0; i < 3 && good; ++i) {
    if (!want[i]) continue;
    char hex[65];
    for (int w = 0; w < 8; ++w) snprintf(hex + 8 * w, 9, "%08x", got[i * 8 + 7 - w]);  // the scalar's words, most significant first
    good = memcmp(hex, want[i], 64) == 0;
  }
  if (!good) {
    h->err = "known-answer test of the key derivation function (ECL_KDF_*) failed";
    return ECL_E_SELFTEST;
  }
  return ECL_OK;
}

extern "C" int ecl_hip_selftest(ecl_hip* h) {
  if (!h) return ECL_E_ARG;
  if (h->gen) {  // the context's own self-test as without the flag (its hash included), then the generator on a built-in template (abi_gen.h)
    h->gen = false;
    const int rc = ecl_hip_selftest(h);
    h->gen = true;
    return rc != ECL_OK ? rc : gen_selftest(h);
  }
  if (h->kdf) {  // the context's own self-test as without the bits, then the hash of its ecl_hip_mul_batch_raw
    const u32 kdf = h->kdf;
    h->kdf = 0;
    const int rc = ecl_hip_selftest(h);
    h->kdf = kdf;
    return rc != ECL_OK ? rc : kdf_selftest(h);
  }
  if (h->bip39) {  // likewise, then both derivation kernels on BIP39's test phrase (abi_seed.h)
    h->bip39 = false;
    const int rc = ecl_hip_selftest(h);
    h->bip39 = true;
    return rc != ECL_OK ? rc : seed_selftest(h);
  }
  if (h->flags & ECL_HERD) {  // a herd context tests the device code a public-key context tests (the known answers, the x-only walk, the
    // window sum); the herd kernel has no second path on the device to be checked against: tests/test_gpu_kangaroo.py checks it
    const u32 offs = h->offs;
    h->flags = ECL_PUB, h->offs = 0;
    const int rc = ecl_hip_selftest(h);
    h->flags = ECL_PUB | ECL_HERD, h->offs = offs;
    return rc;
  }
  // (1) known answers: hash160 of k*G for k = 1, 2, 0xdc2a04 (compressed, uncompressed), public vectors; the P2SH-P2WPKH hash of 1*G
  // (address 3JvL6Ymt8MVWiCNHC7oWU6nLeHNJKLZGLN) and its Ethereum address (7e5f4552091a69125d5dfcb7b8c2659029395bdf)
  static const uint64_t KS[3][4] = {{1, 0, 0, 0}, {2, 0, 0, 0}, {0xdc2a04, 0, 0, 0}};
  static const uint32_t KAT33[3][5] = {{0x751e76e8u, 0x199196d4u, 0x54941c45u, 0xd1b3a323u, 0xf1433bd6u},
                                       {112186475u, 3455918831u, 2494304810u, 2703172626u, 1151565516u},
                                       {156887041u, 569600746u, 330545875u, 1640062380u, 639147567u}};
  static const uint32_t KAT65[3][5] = {{0x91b24bf9u, 0xf5288532u, 0x960ac687u, 0xabb03512u, 0x7b1d28a5u},
                                       {3603490856u, 3253510587u, 2691031480u, 1042137763u, 1849195074u},
                                       {3514751675u, 162192179u, 1444810732u, 2475417333u, 3394525481u}};
  static const uint32_t KATP2SH[5] = {0xbcfeb728u, 0xb584253du, 0x5f3f70bcu, 0xb780e9efu, 0x218a68f4u};
  uint64_t x[3][4], y[3][4];
  uint8_t ok[3];
  static const uint32_t KATETH[5] = {0x7e5f4552u, 0x091a6912u, 0x5d5dfcb7u, 0xb8c26590u, 0x29395bdfu};
  uint32_t h33[3][5], h65[3][5], hsh[1][5], heth[1][5];
  uint8_t oketh[1] = {0};
  // the Taproot output keys of the same three private keys (BIP86 key path; k = 1: bc1pmfr3p9j00pfxjh0zmgp99y8zftmd3s5pmedqhyptwy6lm87hf5sspknck9)
  static const uint32_t KATTR[3][8] = {{0xda471096u, 0x4f785269u, 0x5de2da02u, 0x5290e24au, 0xf6d8c281u, 0xde5a0b90u, 0x2b7135fdu, 0x9fd74d21u},
                                       {0xcafd90c7u, 0x026f0b6au, 0xb98df894u, 0x90d02732u, 0x881f2f4bu, 0x59008563u, 0x58dddff4u, 0x679c2ffbu},
                                       {0x509eeff5u, 0xf103f276u, 0x7a17d328u, 0x9d857dd5u, 0x38a62a94u, 0x49646107u, 0xe5b4b6d0u, 0xa7898714u}};
  uint32_t qtr[3][8];
  uint8_t oktr[3] = {0, 0, 0};
  int rc = ecl_hip_diag_mulg(h, KS, x, y, ok, 3);
  if (rc == ECL_OK) rc = ecl_hip_diag_hash160(h, x, y, h33, h65, 3);
  if (rc == ECL_OK) rc = ecl_hip_p2sh_hash(h, h33, hsh, 1);
  if (rc == ECL_OK) rc = verify_eth_plain(h, KS, 1, heth, oketh);
  if (rc == ECL_OK) rc = ecl_hip_verify_tr(h, KS, 3, qtr, oktr);
  if (rc != ECL_OK) return rc;
  if (memcmp(h33, KAT33, sizeof KAT33) != 0 || memcmp(h65, KAT65, sizeof KAT65) != 0 || memcmp(hsh[0], KATP2SH, sizeof KATP2SH) != 0 ||
      memcmp(heth[0], KATETH, sizeof KATETH) != 0 || !oketh[0] || memcmp(qtr, KATTR, sizeof KATTR) != 0 || !(oktr[0] && oktr[1] && oktr[2]) || !(ok[0] && ok[1] && ok[2])) {
    h->err = "known-answer test of k*G -> hash160 failed";
    return ECL_E_SELFTEST;
  }
  // (2) the walk kernel against the double-and-add kernel: 4096 consecutive keys through an all-ones filter
  const u32 N = 4096, saveB = h->B, saveT = h->Tmax;
  const uint64_t save_cov[3] = {h->cov_requested, h->cov_covered, h->cov_device};  // the caller's totals: "since open" leaves this call out
  const bool saveAuto = h->B_auto;
  // the caller's filter, list and table wait in these three while the context runs the test on its own; swapped back below
  devbuf<u64> keep_bloom;
  devbuf<u32> keep_list, keep_tab;
  const u64 save_words = h->bloom_words, save_list_n = h->list_n;
  const u32 save_prefix_n = h->prefix_n, save_mask_n = h->mask_n, save_tab_B = h->tab_B;
  keep_bloom.swap(h->d_bloom), keep_list.swap(h->d_list), keep_tab.swap(h->d_tab);
  h->bloom_words = 0, h->list_n = 0, h->tab_B = 0;
  // ECL_ORIGIN: the same walk from the origin O = 0xdc2a04 G (its x, y from (1)), against the double-and-add kernel's (start + j s + 0xdc2a04) G;
  // ECL_INSERT: the walk sets bits in a zeroed filter, compared with the filter the host builds from the double-and-add kernel's x
  const bool origin = h->flags & ECL_ORIGIN, insert = h->flags & ECL_INSERT;
  std::vector<u64> ones(insert ? 4099 : 64, insert ? 0ull : ~0ull), got_bits(insert ? 4099 : 0);
  h->B = 16, h->Tmax = 256, h->B_auto = false;
  uint64_t start[12] = {0x0123456789abcdefull, 0x1f, 0, 0};
  memcpy(start + 4, x[2], 32), memcpy(start + 8, y[2], 32);
  const u32 per_key = ((h->flags & ECL_ADDR33) ? 1 : 0) + ((h->flags & ECL_ADDR65) ? 1 : 0) + ((h->flags & ECL_P2SH) ? 1 : 0) +
                      ((h->flags & ECL_ETH) ? 1 : 0) + ((h->flags & ECL_TR) ? 1 : 0) + ((h->flags & ECL_PUB) ? 1 : 0);
  const u32 cap = insert ? 0 : N * per_key * ((h->flags & ECL_ENDO) ? ((h->flags & ECL_PUB) ? 3 : 6) : 1);  // (a public key and its negative share x: three images)
  std::vector<ecl_found> recs(cap);
  u32 n = 0;
  // ECL_PREFIX: the one range [0, 2^160 - 1] stands for the all-ones filter (ten 32-bit words in five 64-bit ones)
  if (h->flags & ECL_PREFIX) {
    ones.assign(5, 0ull);
    ones[2] = ~0ull << 32, ones[3] = ones[4] = ~0ull;
    rc = ecl_hip_set_bloom(h, ones.data(), 5);
  } else if (h->flags & ECL_MASK) {  // ECL_MASK: one entry with an all-zero mask matches every value
    ones.assign(5, 0ull);
    rc = ecl_hip_set_bloom(h, ones.data(), 5);
  } else {
    rc = ecl_hip_set_bloom(h, ones.data(), ones.size());
  }
  if (rc == ECL_OK) rc = ecl_hip_add_range(h, start, N, cap ? recs.data() : nullptr, cap, &n);
  if (rc == ECL_OK && insert) rc = ecl_hip_get_bloom(h, got_bits.data(), got_bits.size());
  std::vector<uint64_t> ks((size_t)N * 4), xs((size_t)N * 4), ys((size_t)N * 4);
  std::vector<uint32_t> r33((size_t)N * 5), r65((size_t)N * 5), rsh((size_t)N * 5), reth((size_t)N * 5);
  std::vector<uint8_t> eok(N);
  std::vector<uint32_t> rtr((h->flags & ECL_TR) ? (size_t)N * 8 : 0);
  const u256 s = sc_pow2(h->offs);
  u256 cur = sc_reduce(u256_from(start));
  if (origin) cur = sc_add(cur, u256_from(KS[2]));
  for (u32 i = 0; i < N; ++i) {
    memcpy(&ks[(size_t)i * 4], cur.w, 32);
    cur = sc_add(cur, s);
  }
  if (rc == ECL_OK) rc = ecl_hip_diag_mulg(h, (const uint64_t(*)[4])ks.data(), (uint64_t(*)[4])xs.data(), (uint64_t(*)[4])ys.data(), nullptr, N);
  if (rc == ECL_OK) rc = ecl_hip_diag_hash160(h, (const uint64_t(*)[4])xs.data(), (const uint64_t(*)[4])ys.data(),
                                              (uint32_t(*)[5])r33.data(), (uint32_t(*)[5])r65.data(), N);
  if (rc == ECL_OK && (h->flags & ECL_P2SH)) rc = ecl_hip_p2sh_hash(h, (const uint32_t(*)[5])r33.data(), (uint32_t(*)[5])rsh.data(), N);
  // an ECL_ETH context: the walk's addresses against the window-table sum's (ecl_hip_verify_eth; (3) checks that sum against the double-and-add kernel)
  if (rc == ECL_OK && (h->flags & ECL_ETH)) rc = verify_eth_plain(h, (const uint64_t(*)[4])ks.data(), N, (uint32_t(*)[5])reth.data(), eok.data());
  // an ECL_TR context: the walk's and k_tr_check's output keys against the window-table path's (ecl_hip_verify_tr)
  if (rc == ECL_OK && (h->flags & ECL_TR)) rc = ecl_hip_verify_tr(h, (const uint64_t(*)[4])ks.data(), N, (uint32_t(*)[8])rtr.data(), eok.data());
  // an ECL_PUB context: the walk's x against the double-and-add kernel's, its leading 20 bytes as five big-endian words
  std::vector<uint32_t> rpub((h->flags & ECL_PUB) ? (size_t)N * 5 : 0);
  if (h->flags & ECL_PUB)
    for (u32 i = 0; i < N; ++i)
      for (u32 j = 0; j < 5; ++j) rpub[(size_t)i * 5 + j] = (uint32_t)(xs[(size_t)i * 4 + (7 - j) / 2] >> (32 * ((7 - j) & 1)));
  // restore the caller's state whatever happened; the test's own filter and table are freed here, not at the end of the function
  keep_bloom.swap(h->d_bloom), keep_list.swap(h->d_list), keep_tab.swap(h->d_tab);
  keep_bloom.reset(), keep_tab.reset();
  h->bloom_words = save_words, h->prefix_n = save_prefix_n, h->mask_n = save_mask_n, h->list_n = save_list_n, h->tab_B = save_tab_B;
  h->B = saveB, h->Tmax = saveT, h->B_auto = saveAuto;
  h->walk_valid = false;
  h->kernel_ms = 0, h->launches = 0, h->keys = 0, h->setup_ms = 0, h->setups = 0;
  h->cov_requested = save_cov[0], h->cov_covered = save_cov[1], h->cov_device = save_cov[2];
  if (rc != ECL_OK) return rc;
  if (insert) {
    const bloom_t bl = bloom_make(nullptr, ones.size());
    for (u32 i = 0; i < N; ++i) {
      u64 a[5];
      bloom_words_of(a, &rpub[(size_t)i * 5]);
      for (int p = 0; p < 20; ++p) {
        const u64 idx = bloom_index(a, p);
        ones[bloom_mod(bl, idx >> 6)] |= 1ull << (idx & 63);
      }
    }
    if (n != 0 || ones != got_bits) {
      h->err = "the filter the insert walk built disagrees with the double-and-add kernel's";
      return ECL_E_SELFTEST;
    }
  }
  u32 seen = insert ? N * per_key : 0;
  bool good = n == cap;
  for (u32 i = 0; i < n && good; ++i) {
    const ecl_found& f = recs[i];
    if (f.key_offset >= N) { good = false; break; }
    if (f.endo != 0) continue;  // the endomorphism images are covered by the parity tests; here: the walk itself
    const uint32_t* want = f.compressed == 5 ? &rpub[f.key_offset * 5] : f.compressed == 4 ? &rtr[f.key_offset * 8] : f.compressed == 3 ? &reth[f.key_offset * 5] : f.compressed == 2 ? &rsh[f.key_offset * 5] : f.compressed ? &r33[f.key_offset * 5] : &r65[f.key_offset * 5];
    good = memcmp(f.h160, want, 20) == 0;
    ++seen;
  }
  if (!good || seen != N * per_key) {
    h->err = "walk kernel disagrees with the double-and-add kernel";
    return ECL_E_SELFTEST;
  }
  // (3) the window-table sum (gtable_mul: ecl_hip_verify, the base centre of every non-contiguous walk, `mul`) against the
  // double-and-add kernel on full-width scalars, so that every one of the 19 windows carries a digit: the walk's base
  // centre and the verification of its hits share this function and the table, and a hit shares its high digits with
  // the base centre - (2) exercises only the low windows.  Scalars: a fixed xorshift stream, plus every digit at its
  // maximum (0x3fff in all windows) and a single top-window digit.
  {
    const u32 M = 48;
    std::vector<uint64_t> vk((size_t)M * 4), vx((size_t)M * 4), vy((size_t)M * 4);
    std::vector<uint32_t> w33((size_t)M * 5), w65((size_t)M * 5), g33((size_t)M * 5), g65((size_t)M * 5);
    std::vector<uint8_t> vok(M), gok(M);
    u64 z = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < vk.size(); ++i) {
      z ^= z << 13, z ^= z >> 7, z ^= z << 17;
      vk[i] = z;
    }
    for (int w = 0; w < 4; ++w) vk[w] = ~0ull;                 // all digits 0x3fff (the sum is (2^256 - 1) mod n times G)
    vk[4] = 0, vk[5] = 0, vk[6] = 0, vk[7] = 1ull << 60;       // window 18 only
    rc = verify_plain(h, (const uint64_t(*)[4])vk.data(), M, (uint32_t(*)[5])g33.data(), (uint32_t(*)[5])g65.data(), gok.data());
    if (rc == ECL_OK) rc = ecl_hip_diag_mulg(h, (const uint64_t(*)[4])vk.data(), (uint64_t(*)[4])vx.data(), (uint64_t(*)[4])vy.data(), vok.data(), M);
    if (rc == ECL_OK) rc = ecl_hip_diag_hash160(h, (const uint64_t(*)[4])vx.data(), (const uint64_t(*)[4])vy.data(),
                                                (uint32_t(*)[5])w33.data(), (uint32_t(*)[5])w65.data(), M);
    if (rc != ECL_OK) return rc;
    if (g33 != w33 || g65 != w65 || gok != vok) {
      h->err = "window-table scalar multiplication disagrees with the double-and-add kernel";
      return ECL_E_SELFTEST;
    }
  }
  return ECL_OK;
}
