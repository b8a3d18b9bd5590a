// gen_host.cpp — compiles the candidate generator of the DEVICE header gen.h (the body of k_gen_lines) and the host's template code
// (host/gen_plan.h: the validator, the builder, the mask parser, the host's own expansion by division) for the host with g++, so that the
// CPU test-suite can check them without a GPU (tests/test_brain_host.py).  Built as a shared object for the tests; it has a main of its
// own as well - a few templates expanded both ways in heap blocks of exactly the sizes the library gives the device - so the same code
// can be built as a program under a sanitizer and run directly: a gather behind the table's spare words or a store outside a
// candidate's slot would be a heap overflow there.  Not part of the product library.
#include "../gen.h"
#include "../../host/gen_plan.h"
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

// (the kernel's arguments, the slot size and the table's size are gen.h's: what the library uses)
static gen_args args_of(const gen_info& gi) { return gen_args_make(gi.npos, gi.alt_at, gi.pool_at, gi.count, gi.first); }

extern "C" {
// the validator: 0 and T, L, or -1 and the reason in why[160]
int gh_check(const u8* blob, size_t bytes, unsigned long long* T, u32* L, char* why) {
  gen_info gi;
  const char* w = gen_blob_check(blob, bytes, &gi);
  if (w) return snprintf(why, 160, "%s", w), -1;
  *T = gi.T, *L = gi.L;
  return 0;
}
u32 gh_threads_r(void) { return GEN_R; }
// what a k_gen_lines launch over the m candidates first ... first + m - 1 writes: text (m * stride bytes + 8 spare, stride = L in whole
// words, at least 4) and the line table; thread by thread, as the kernel does it.  -> the stride, 0 for a refused blob
u32 gh_device_lines(const u8* blob, size_t bytes, unsigned long long first, u32 m, u8* text_out, unsigned long long* lines_out) {
  gen_info gi;
  if (gen_blob_check(blob, bytes, &gi)) return 0;
  const u32 stride = gen_stride_bytes(gi.L);
  // the table and the text in heap blocks of exactly the library's sizes
  const size_t tab_words = gen_table_words(bytes), text_words = (size_t)m * stride / 4 + 2;
  u32* tab = (u32*)calloc(tab_words, 4);
  u32* text = (u32*)calloc(text_words, 4);
  u64* lines = (u64*)calloc(m ? m : 1, 8);
  memcpy(tab, blob, bytes);
  const gen_args g = args_of(gi);
  const u32 threads = (m + GEN_R - 1u) / GEN_R;
  for (u32 t = 0; t < (threads + 255u) / 256u * 256u; ++t) gen_thread(tab, g, first, m, t, stride, 0, text, lines);
  memcpy(text_out, text, (size_t)m * stride);
  for (u32 j = 0; j < m; ++j) lines_out[j] = lines[j];
  free(tab), free(text), free(lines);
  return stride;
}
// the host's own expansion: candidate i into out[256] -> its length, or -1 for a refused blob or an index outside the template
int gh_host_candidate(const u8* blob, size_t bytes, unsigned long long i, u8* out) {
  gen_info gi;
  if (gen_blob_check(blob, bytes, &gi) || i >= gi.T) return -1;
  return (int)gen_candidate_host(blob, &gi, i, out);
}
// the command line's mask and sets (sets[k]: the text of -<k + 1>, or NULL) -> the blob's length (copied to blob_out if it fits cap),
// or -1 and the reason in why[320]
long gh_parse_mask(const char* mask, const char* const sets[4], u8* blob_out, size_t cap, char* why) {
  gen_build built[4], out;
  const gen_build* use[4] = {nullptr, nullptr, nullptr, nullptr};
  memset(built, 0, sizeof built);
  long r = -1;
  bool ok = true;
  for (int k = 0; k < 4 && ok; ++k)
    if (sets[k]) {
      ok = gen_parse_set(sets[k], (char)('1' + k), &built[k], why, 320) == 0;
      use[k] = &built[k];
    }
  memset(&out, 0, sizeof out);
  if (ok && gen_parse_mask(mask, use, &out, why, 320) == 0) {
    size_t bytes = 0;
    u8* blob = gen_build_blob(&out, &bytes);
    if (blob) {
      r = (long)bytes;
      if (bytes <= cap) memcpy(blob_out, blob, bytes);
      free(blob);
    } else snprintf(why, 320, "out of memory");
  }
  for (int k = 0; k < 4; ++k) gen_build_free(&built[k]);
  gen_build_free(&out);
  return r;
}
}

static int fail(const char* what) { return printf("%s failed\n", what), 1; }
// every candidate of [first, first + m) both ways, against each other
static bool both_ways(const std::vector<u8>& blob, u64 first, u32 m, std::vector<std::string>* got = nullptr) {
  gen_info gi;
  if (gen_blob_check(blob.data(), blob.size(), &gi)) return false;
  const u32 stride = gen_stride_bytes(gi.L);
  std::vector<u8> text((size_t)m * stride + 8);
  std::vector<unsigned long long> lines(m);
  if (gh_device_lines(blob.data(), blob.size(), first, m, text.data(), lines.data()) != stride) return false;
  for (u32 j = 0; j < m; ++j) {
    u8 want[GEN_L_MAX];
    const u32 len = gen_candidate_host(blob.data(), &gi, first + j, want);
    if ((u32)lines[j] != j * stride || (u32)(lines[j] >> 32) != len || memcmp(text.data() + (u32)lines[j], want, len)) return false;
    if (got) got->push_back(std::string((const char*)want, len));
  }
  return true;
}
static std::vector<u8> blob_of(const std::vector<std::vector<std::string>>& positions) {
  gen_build b;
  memset(&b, 0, sizeof b);
  for (const auto& pos : positions) {
    gen_build_pos(&b);
    for (const auto& a : pos) gen_build_alt(&b, (const u8*)a.data(), a.size());
  }
  size_t bytes = 0;
  u8* blob = gen_build_blob(&b, &bytes);
  gen_build_free(&b);
  std::vector<u8> v(blob, blob + bytes);
  free(blob);
  return v;
}
int main() {
  {  // the library's self-test template, all of it, from every start
    const auto blob = blob_of({{"ab", "c"}, {"", "xyz"}, {"-"}, {"0", "1", "2"}});
    static const char* const WANT[12] = {"ab-0", "ab-1", "ab-2", "abxyz-0", "abxyz-1", "abxyz-2", "c-0", "c-1", "c-2", "cxyz-0", "cxyz-1", "cxyz-2"};
    for (u32 first = 0; first < 12; ++first) {
      std::vector<std::string> got;
      if (!both_ways(blob, first, 12 - first, &got)) return fail("the small template");
      for (u32 j = 0; j < 12 - first; ++j)
        if (got[j] != WANT[first + j]) return fail("the small template's text");
    }
  }
  {  // L = 256 from a 255-byte word and a byte; a 0-byte alternative beside it; radices 1 and 2 through 16 positions
    const auto blob = blob_of({{std::string(255, 'x'), ""}, {"y", "z"}});
    if (!both_ways(blob, 0, 4)) return fail("L = 256");
    std::vector<std::vector<std::string>> pos;
    for (int p = 0; p < 16; ++p) pos.push_back(p % 3 == 1 ? std::vector<std::string>{"-"} : std::vector<std::string>{"a", "bc"});
    const auto carry = blob_of(pos);
    if (!both_ways(carry, 0, 2048)) return fail("sixteen positions");
  }
  {  // T = 2^56 - 2^24 from four radices: the last candidates, and indices around 2^32 (where the digits' division changes its width)
    std::vector<std::vector<std::string>> pos(4);
    const u32 radix[4] = {65535u, 65537u, 256u, 16777216u / 256u};  // 65535 * 65537 = 2^32 - 1; * 2^8 * 2^16 = 2^56 - 2^24
    for (int p = 0; p < 4; ++p)
      for (u32 a = 0; a < radix[p]; ++a) pos[p].push_back(std::to_string(a % 1000u).substr(0, 1 + a % 3u));
    const auto blob = blob_of(pos);
    gen_info gi;
    if (gen_blob_check(blob.data(), blob.size(), &gi) || gi.T != ((1ull << 56) - (1ull << 24))) return fail("the wide template");
    if (!both_ways(blob, (1ull << 32) - 7, 19) || !both_ways(blob, gi.T - 13, 13)) return fail("wide indices");
  }
  {  // the mask parser, and a refused blob
    const char* sets[4] = {"ab?d", nullptr, nullptr, nullptr};
    u8 blob[4096];
    char why[320];
    const long n = gh_parse_mask("x?1??y?d", sets, blob, sizeof blob, why);
    unsigned long long T;
    u32 L;
    if (n < 0 || gh_check(blob, (size_t)n, &T, &L, why) != 0 || T != 120 || L != 5) return fail("the mask parser");
    blob[5] = 1;
    if (gh_check(blob, (size_t)n, &T, &L, why) == 0) return fail("the validator");
    if (gh_parse_mask("?1?2", sets, blob, sizeof blob, why) != -1) return fail("a set that is not given");
  }
  puts("ok");
  return 0;
}
