// callstate.h - what a search call (add_range, mul_batch, mul_batch_raw) leaves behind, without the device: the names of the counter
// words, the one owner of "where the last call's records are", and the verdict of a call as a pure function of the words read back.
// No HIP header, like devbuf.h: compiles for the host alone (tools/callstate_host.cpp walks the verdict through a table of cases).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <memory>

#include "../../include/ecloop_hip.h"

// d_counter / pin_counter: eight words the kernels write (zeroed in front of every call, read back once behind it) and a ninth that only
// the host copy has
enum : uint32_t {
  CW_PUSHED = 0,       // records appended by the search kernel
  CW_CONFIRMED = 1,    // records confirmed by the list (k_list_filter)
  CW_RAW_OUTSIDE = 2,  // mul_batch_raw: a line lies outside the text
  CW_RAW_LATE = 3,     // mul_batch_raw: a line beyond the part of the text that was on the device when it was hashed
  CW_KEYS = 4,         // u64 (4, 5): keys hashed; Taproot: points emitted; the herd: jumps made
  CW_TR_CHECKED = 6,   // u64 (6, 7): Taproot: slab entries that reached k_tr_check's probe step
  CW_HERD_FLAGS = 6,   // the SAME word on a herd context (never Taproot): bit 0 a distance passed 2^128, bit 1 a start at infinity
  CW_DEVICE_WORDS = 8,
  CW_ORIGIN_INF = 8,   // host copy only: k_origin_add's flag (origin + base point = the point at infinity), copied from behind d_aux
  CW_HOST_WORDS = 9
};
static inline uint64_t cw_u64(const uint32_t* w, uint32_t at) { return (uint64_t)w[at] | (uint64_t)w[at + 1] << 32; }
static inline uint64_t counted_keys(const uint32_t* w) { return cw_u64(w, CW_KEYS); }
static inline uint64_t tr_checked_keys(const uint32_t* w) { return cw_u64(w, CW_TR_CHECKED); }
static inline bool raw_line_outside(const uint32_t* w) { return w[CW_RAW_OUTSIDE] != 0; }
static inline bool raw_line_late(const uint32_t* w) { return w[CW_RAW_LATE] != 0; }
static inline uint32_t herd_flags(const uint32_t* w) { return w[CW_HERD_FLAGS]; }
#define HERD_FLAG_DISTANCE 1u
#define HERD_FLAG_INFINITY 2u

// Where the records of the last call are (ecl_hip_fetch_found): nowhere, in the device's record buffer - from `at`, `held` of the call's
// `total`, the endo byte meaningful or not - or in a look-ahead sweep on the host (`n` records from `host_at` of the region, key offsets
// counted from `off`).  The three transitions are the only writers.
struct la_region;
struct last_records {
  uint32_t at = 0, held = 0, total = 0;
  bool endo = false, from_host = false;
  std::shared_ptr<la_region> region;
  size_t host_at = 0;
  uint32_t n = 0;
  uint64_t off = 0;
  void forget() { held = total = n = 0, from_host = false, region.reset(); }
  void on_device(uint32_t at_, uint32_t held_, uint32_t total_, bool endo_) { forget(), at = at_, held = held_, total = total_, endo = endo_; }
  void on_host(std::shared_ptr<la_region> r, size_t at_, uint32_t n_, uint64_t off_) { forget(), region = std::move(r), host_at = at_, n = n_, off = off_, from_host = true; }
};

// The verdict of a call, from the nine words read back.  cap: records the caller takes; rcap: records the device keeps (>= cap); list: the
// confirmed records count, and start at rcap; want: keys asked for; want2: null, or the second count asked for (Taproot).
enum call_text { TEXT_NONE, TEXT_LIST_OVERFLOW, TEXT_SHORT, TEXT_SHORT2 };
struct call_verdict {
  int rc;               // ECL_OK, ECL_E_OVERFLOW or ECL_E_COVERAGE
  uint32_t nout;        // *nout
  uint32_t take, from;  // records to copy to the caller, and where they start in the record buffer
  uint32_t held, total; // the last records: on the device from `from` - unless rc is ECL_E_COVERAGE: forgotten
  call_text text;       // the error text that applies
  uint64_t got;         // TEXT_SHORT / TEXT_SHORT2: the count that fell short (or long)
};
static inline call_verdict call_verdict_of(const uint32_t* w, uint32_t cap, uint32_t rcap, bool list, uint64_t want, const uint64_t* want2) {
  const uint32_t cnt = list ? w[CW_CONFIRMED] : w[CW_PUSHED];
  call_verdict v = {cnt > cap ? ECL_E_OVERFLOW : ECL_OK, cnt, cnt < cap ? cnt : cap, list ? rcap : 0, cnt < rcap ? cnt : rcap, cnt, TEXT_NONE, 0};
  if (list && w[CW_PUSHED] > rcap)  // the bloom let more through than the staging area holds: some were never looked up, so nothing to fetch
    v.rc = ECL_E_OVERFLOW, v.nout = w[CW_PUSHED], v.held = 0, v.total = w[CW_PUSHED], v.text = TEXT_LIST_OVERFLOW;
  const bool short1 = counted_keys(w) != want;
  if (short1 || (want2 && tr_checked_keys(w) != *want2))  // no records, nothing to fetch
    v.rc = ECL_E_COVERAGE, v.nout = 0, v.held = v.total = 0, v.text = short1 ? TEXT_SHORT : TEXT_SHORT2, v.got = short1 ? counted_keys(w) : tr_checked_keys(w);
  return v;
}
// the text of ecl_hip_last_error for a verdict (what / what2: the call's name in TEXT_SHORT / TEXT_SHORT2); false: the verdict has none
static inline bool call_verdict_text(const call_verdict& v, const char* what, const char* what2, uint64_t want, char* msg, size_t len) {
  if (v.text == TEXT_LIST_OVERFLOW) snprintf(msg, len, "list mode: more bloom hits in one call than the device staging area holds");
  if (v.text == TEXT_SHORT || v.text == TEXT_SHORT2)
    snprintf(msg, len, "%s: the device hashed %llu keys of the %llu asked for", v.text == TEXT_SHORT ? what : what2, (unsigned long long)v.got, (unsigned long long)want);
  return v.text != TEXT_NONE;
}
// the totals of ecl_hip_get_coverage by a call's result: one that returns ECL_OK / ECL_E_OVERFLOW was launched or served and counted whole;
// one that returns ECL_E_COVERAGE was launched and not; any other was refused
static inline bool rc_was_launched(int rc) { return rc == ECL_OK || rc == ECL_E_OVERFLOW || rc == ECL_E_COVERAGE; }
static inline bool rc_was_whole(int rc) { return rc == ECL_OK || rc == ECL_E_OVERFLOW; }
