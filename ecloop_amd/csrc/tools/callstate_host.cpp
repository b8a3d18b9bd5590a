// callstate_host.cpp - the verdict of a search call (csrc/callstate.h, verbatim) on the host: a table of counter words walked through
// call_verdict_of, every output field compared, the texts, the last-records transitions and the coverage totals by result.  A program of
// its own, meant to be built with the address and undefined-behaviour sanitizers (tests/test_callstate_host.py).
#include <stdio.h>
#include <string.h>

#include "../callstate.h"
struct la_region {
  int dummy = 0;
};

static int failed = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) printf("line %d: %s\n", __LINE__, #cond), failed = 1;    \
  } while (0)

struct verdict_case {
  const char* name;
  uint32_t pushed, confirmed;
  uint64_t keys, checked;  // the two counts read back
  uint32_t cap, rcap;
  bool list, second;       // second: the second count is asked for too
  call_verdict want;
  const char* text;        // of ecl_hip_last_error; null: none
};
static const uint64_t N = 1000;  // keys asked for
static const char LIST_TEXT[] = "list mode: more bloom hits in one call than the device staging area holds";
static const verdict_case CASES[] = {
    // without a list: the pushed records count, they start at 0
    {"cnt < cap", 5, 0, N, 0, 8, 20, false, false, {ECL_OK, 5, 5, 0, 5, 5, TEXT_NONE, 0}, nullptr},
    {"cnt == cap", 8, 0, N, 0, 8, 20, false, false, {ECL_OK, 8, 8, 0, 8, 8, TEXT_NONE, 0}, nullptr},
    {"cap < cnt <= rcap", 20, 0, N, 0, 8, 20, false, false, {ECL_E_OVERFLOW, 20, 8, 0, 20, 20, TEXT_NONE, 0}, nullptr},
    {"cnt > rcap", 21, 0, N, 0, 8, 20, false, false, {ECL_E_OVERFLOW, 21, 8, 0, 20, 21, TEXT_NONE, 0}, nullptr},
    {"no list: the confirmed word is not looked at", 5, 99, N, 0, 8, 20, false, false, {ECL_OK, 5, 5, 0, 5, 5, TEXT_NONE, 0}, nullptr},
    // with a list: the confirmed records count, they start at rcap
    {"list, cnt < cap", 20, 5, N, 0, 8, 20, true, false, {ECL_OK, 5, 5, 20, 5, 5, TEXT_NONE, 0}, nullptr},
    {"list, cnt == cap", 20, 8, N, 0, 8, 20, true, false, {ECL_OK, 8, 8, 20, 8, 8, TEXT_NONE, 0}, nullptr},
    {"list, cap < cnt <= rcap", 20, 20, N, 0, 8, 20, true, false, {ECL_E_OVERFLOW, 20, 8, 20, 20, 20, TEXT_NONE, 0}, nullptr},
    {"list, cnt > rcap", 20, 21, N, 0, 8, 20, true, false, {ECL_E_OVERFLOW, 21, 8, 20, 20, 21, TEXT_NONE, 0}, nullptr},
    {"list, pushed > rcap: nothing fetchable", 21, 5, N, 0, 8, 20, true, false, {ECL_E_OVERFLOW, 21, 5, 20, 0, 21, TEXT_LIST_OVERFLOW, 0}, LIST_TEXT},
    // the counts
    {"keys short by one", 5, 0, N - 1, 0, 8, 20, false, false, {ECL_E_COVERAGE, 0, 5, 0, 0, 0, TEXT_SHORT, N - 1}, "one: the device hashed 999 keys of the 1000 asked for"},
    {"keys long by one", 5, 0, N + 1, 0, 8, 20, false, false, {ECL_E_COVERAGE, 0, 5, 0, 0, 0, TEXT_SHORT, N + 1}, "one: the device hashed 1001 keys of the 1000 asked for"},
    {"keys short past the cap and the list's staging area", 21, 9, 7, 0, 8, 20, true, false, {ECL_E_COVERAGE, 0, 8, 20, 0, 0, TEXT_SHORT, 7}, "one: the device hashed 7 keys of the 1000 asked for"},
    {"second count short, first whole", 5, 0, N, N - 3, 8, 20, false, true, {ECL_E_COVERAGE, 0, 5, 0, 0, 0, TEXT_SHORT2, N - 3}, "two: the device hashed 997 keys of the 1000 asked for"},
    {"both short: the first is named", 5, 0, 1, 2, 8, 20, false, true, {ECL_E_COVERAGE, 0, 5, 0, 0, 0, TEXT_SHORT, 1}, "one: the device hashed 1 keys of the 1000 asked for"},
    {"second count not asked for", 5, 0, N, 0, 8, 20, false, false, {ECL_OK, 5, 5, 0, 5, 5, TEXT_NONE, 0}, nullptr},
    {"both whole", 5, 0, N, N, 8, 20, false, true, {ECL_OK, 5, 5, 0, 5, 5, TEXT_NONE, 0}, nullptr},
    {"a count above 2^32", 0, 0, (1ull << 32) + 5, 0, 8, 20, false, false, {ECL_E_COVERAGE, 0, 0, 0, 0, 0, TEXT_SHORT, (1ull << 32) + 5}, "one: the device hashed 4294967301 keys of the 1000 asked for"},
    // cap == 0: nothing is copied, any record is one too many
    {"cap == 0, no records", 0, 0, N, 0, 0, 20, false, false, {ECL_OK, 0, 0, 0, 0, 0, TEXT_NONE, 0}, nullptr},
    {"cap == 0, records", 3, 0, N, 0, 0, 20, false, false, {ECL_E_OVERFLOW, 3, 0, 0, 3, 3, TEXT_NONE, 0}, nullptr},
};

int main() {
  int ran = 0;
  for (const verdict_case& c : CASES) {
    uint32_t w[CW_HOST_WORDS] = {};
    w[CW_PUSHED] = c.pushed, w[CW_CONFIRMED] = c.confirmed;
    w[CW_KEYS] = (uint32_t)c.keys, w[CW_KEYS + 1] = (uint32_t)(c.keys >> 32);
    w[CW_TR_CHECKED] = (uint32_t)c.checked, w[CW_TR_CHECKED + 1] = (uint32_t)(c.checked >> 32);
    w[CW_RAW_OUTSIDE] = 7, w[CW_ORIGIN_INF] = 1;  // (words the verdict does not depend on)
    const call_verdict v = call_verdict_of(w, c.cap, c.rcap, c.list, N, c.second ? &N : nullptr);
    const call_verdict& e = c.want;
    const bool same = v.rc == e.rc && v.nout == e.nout && v.take == e.take && v.from == e.from && v.held == e.held && v.total == e.total &&
                      v.text == e.text && v.got == e.got;
    if (!same)
      printf("%s: rc %d nout %u take %u from %u held %u total %u text %d got %llu\n", c.name, v.rc, v.nout, v.take, v.from, v.held, v.total, (int)v.text,
             (unsigned long long)v.got),
          failed = 1;
    char msg[160] = "untouched";
    const bool has = call_verdict_text(v, "one", "two", N, msg, sizeof msg);
    if (has != (c.text != nullptr) || strcmp(msg, c.text ? c.text : "untouched") != 0) printf("%s: text \"%s\"\n", c.name, msg), failed = 1;
    CHECK(v.take <= c.cap && v.held <= c.rcap && v.from + v.held <= (c.list ? 2 : 1) * c.rcap);  // never past either buffer
    ++ran;
  }
  // the accessors
  {
    uint32_t w[CW_HOST_WORDS] = {1, 2, 0, 4, 0x55, 0x66, 0x77, 0x88, 9};
    CHECK(counted_keys(w) == 0x6600000055ull && tr_checked_keys(w) == 0x8800000077ull && herd_flags(w) == 0x77);
    CHECK(!raw_line_outside(w) && raw_line_late(w));
    CHECK(CW_HERD_FLAGS == CW_TR_CHECKED && CW_ORIGIN_INF == CW_DEVICE_WORDS && CW_HOST_WORDS == CW_DEVICE_WORDS + 1);
  }
  // the last records: each transition leaves nothing of the state before
  {
    last_records l;
    CHECK(l.held == 0 && !l.from_host && !l.region);
    l.on_device(20, 7, 9, true);
    CHECK(l.at == 20 && l.held == 7 && l.total == 9 && l.endo && !l.from_host && !l.region);
    auto r = std::make_shared<la_region>();
    l.on_host(r, 3, 5, 100);
    CHECK(l.from_host && l.region == r && l.host_at == 3 && l.n == 5 && l.off == 100 && l.held == 0 && l.total == 0 && r.use_count() == 2);
    l.on_device(0, 1, 1, false);
    CHECK(!l.from_host && !l.region && l.n == 0 && l.held == 1 && !l.endo && r.use_count() == 1);
    l.on_host(r, 0, 2, 0);
    l.forget();
    CHECK(!l.from_host && !l.region && l.n == 0 && l.held == 0 && l.total == 0 && r.use_count() == 1);
  }
  // the coverage totals by result
  for (int rc = ECL_E_COVERAGE - 2; rc <= 1; ++rc) {
    CHECK(rc_was_launched(rc) == (rc == ECL_OK || rc == ECL_E_OVERFLOW || rc == ECL_E_COVERAGE));
    CHECK(rc_was_whole(rc) == (rc == ECL_OK || rc == ECL_E_OVERFLOW));
  }
  if (failed) return 1;
  printf("callstate_host: ok (%d cases)\n", ran);
  return 0;
}
