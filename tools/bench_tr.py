#!/usr/bin/env python3
"""Taproot (`-a t`) rates on one GPU, in one process, profiler off (profiles/r08_tr.txt):
  a  ecl_hip_add_range on a Taproot context over 2^32 keys (HIP-event rate of both stages, and the wall-clock rate of the call);
  b  ecl_hip_mul_batch with ECL_ADDR33 on 2^26-scalar calls from page-locked memory - the yardstick: the unchanged `mul` kernel;
  c  ecl_hip_mul_batch with ECL_TR on the same calls;
all at the 26-bit window table (what a 2^32-key Taproot call takes by itself), warm, `runs` alternating rounds, medians reported.
A design-density synthetic filter (56 MB, bit density 0.375), look-ahead off.

usage: bench_tr.py rates [runs = 3] [log2 keys of a = 32] [log2 scalars of b, c = 26]
       bench_tr.py add <log2 keys>      one warm-up call and one Taproot add_range call of that size (for a profiler run of its own)"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ecloop_amd import capi  # noqa: E402
from synth import synth_bloom_words  # noqa: E402

START = 0x4000_0000_0000
WINDOW = 26


def context(**kw):
    d = capi.Device(0, **kw)
    d.set_bloom(synth_bloom_words(7000003, 23, "a&(b|c)"))
    d.set_lookahead(0)
    d.set_mul_window(WINDOW)
    return d


def timed_add(d, start, n):
    ms0 = d.timing()[0]
    t0 = time.perf_counter()
    recs, total = d.add_range(start, n, cap=1 << 16)
    wall = time.perf_counter() - t0
    return (d.timing()[0] - ms0) * 1e-3, wall, total


def timed_mul(d, ptr, n, out, cnt):
    ms0 = d.mul_timing()[0]
    t0 = time.perf_counter()
    rc = d.lib.ecl_hip_mul_batch(d.h, ptr, n, out.ctypes.data, len(out), C.byref(cnt))
    wall = time.perf_counter() - t0
    assert rc == 0, rc
    return (d.mul_timing()[0] - ms0) * 1e-3, wall, cnt.value


def rates(runs, la, lm):
    na, nm = 1 << la, 1 << lm
    tr, c33 = context(a33=False, tr=True), context(a33=True)
    ptr = tr.lib.ecl_hip_alloc_host(nm * 32)
    assert ptr
    K = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(nm, 4))
    K[:] = np.random.RandomState(1).randint(0, 1 << 63, size=(nm, 4), dtype=np.int64).astype(np.uint64)
    out, cnt = np.zeros(1 << 16, dtype=capi.FOUND_DTYPE), C.c_uint32()
    timed_add(tr, START - (1 << 28), 1 << 28)  # warm: tables, buffers, code objects
    timed_mul(c33, ptr, nm, out, cnt), timed_mul(tr, ptr, nm, out, cnt)
    rows = {"a": [], "b": [], "c": []}
    for r in range(runs):
        rows["a"].append(timed_add(tr, START + r * na, na))
        rows["b"].append(timed_mul(c33, ptr, nm, out, cnt))
        rows["c"].append(timed_mul(tr, ptr, nm, out, cnt))
    res = {"runs": runs, "window_bits": tr.mul_window(), "keys_a": na, "scalars_bc": nm}
    for leg, n in (("a", na), ("b", nm), ("c", nm)):
        res[leg] = {"event_M_per_s": [round(n / e / 1e6, 1) for e, _, _ in rows[leg]], "wall_M_per_s": [round(n / w / 1e6, 1) for _, w, _ in rows[leg]],
                    "event_median_M_per_s": round(statistics.median(n / e / 1e6 for e, _, _ in rows[leg]), 1),
                    "wall_median_M_per_s": round(statistics.median(n / w / 1e6 for _, w, _ in rows[leg]), 1), "hits": [h for _, _, h in rows[leg]]}
    res["a_over_b_event"] = round(res["a"]["event_median_M_per_s"] / res["b"]["event_median_M_per_s"], 3)
    res["c_over_b_event"] = round(res["c"]["event_median_M_per_s"] / res["b"]["event_median_M_per_s"], 3)
    res["coverage_tr"] = tr.coverage()
    tr.lib.ecl_hip_free_host(ptr)
    tr.close(), c33.close()
    print(json.dumps(res))


def one_add(log2):
    d = context(a33=False, tr=True)
    timed_add(d, START - (1 << 26), 1 << 26)
    ev, wall, total = timed_add(d, START, 1 << log2)
    print(json.dumps({"keys": 1 << log2, "event_s": round(ev, 4), "wall_s": round(wall, 4), "event_M_per_s": round((1 << log2) / ev / 1e6, 1), "hits": total,
                      "window_bits": d.mul_window()}))
    d.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "add":
        one_add(int(sys.argv[2]))
    elif len(sys.argv) > 1 and sys.argv[1] == "rates":
        rates(int(sys.argv[2]) if len(sys.argv) > 2 else 3, int(sys.argv[3]) if len(sys.argv) > 3 else 32, int(sys.argv[4]) if len(sys.argv) > 4 else 26)
    else:
        sys.exit(__doc__)
