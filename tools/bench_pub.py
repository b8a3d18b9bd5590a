#!/usr/bin/env python3
"""Public-key (`-a x`) rates on one GPU, in one process, profiler off (profiles/r09_pub.txt):
  c   ecl_hip_add_range with ECL_ADDR33 over 2^32 keys - the yardstick: the unchanged addr33 kernel of this build;
  x   the same call with ECL_PUB;
  xe  the same call with ECL_PUB | ECL_ENDO (keys WALKED per second; the status line counts six per key);
  mc  ecl_hip_mul_batch with ECL_ADDR33 on 2^26-scalar calls from page-locked memory;
  mx  the same calls with ECL_PUB;
warm, `runs` alternating rounds, medians reported.  A design-density synthetic filter (bit density 0.375) of `filter words` 64-bit words
(default 7000003: the bench's 56 MB; 2^29 for a 4 GB filter whose every probe is a random HBM sector), look-ahead off, 2^20 lanes per
context (the half group stays automatic).

usage: bench_pub.py rates [runs = 3] [log2 keys = 32] [log2 scalars = 26] [filter words = 7000003]
       bench_pub.py add <log2 keys> [endo]   one warm-up call and one pub add_range call of that size (for a profiler run of its own)"""
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


def context(words, **kw):
    d = capi.Device(0, **kw)
    d.set_bloom(words)
    d.set_lookahead(0)
    d.set_geometry(0, 1 << 20)  # three contexts side by side: 2^20 lanes each (38 GB of chains) so that none is cut back for want of memory
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


def rates(runs, la, lm, nwords):
    na, nm = 1 << la, 1 << lm
    words = synth_bloom_words(nwords, 23, "a&(b|c)")
    ctx = {"c": context(words, a33=True), "x": context(words, a33=False, pub=True), "xe": context(words, a33=False, pub=True, endo=True)}
    del words
    ptr = ctx["c"].lib.ecl_hip_alloc_host(nm * 32)
    assert ptr
    K = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(nm, 4))
    K[:] = np.random.RandomState(1).randint(0, 1 << 63, size=(nm, 4), dtype=np.int64).astype(np.uint64)
    out, cnt = np.zeros(1 << 16, dtype=capi.FOUND_DTYPE), C.c_uint32()
    for d in ctx.values():  # warm: tables, buffers, code objects
        timed_add(d, START - (1 << 28), 1 << 28)
    timed_mul(ctx["c"], ptr, nm, out, cnt), timed_mul(ctx["x"], ptr, nm, out, cnt)
    rows = {k: [] for k in ("c", "x", "xe", "mc", "mx")}
    for r in range(runs):
        for leg in ("c", "x", "xe"):
            rows[leg].append(timed_add(ctx[leg], START + r * na, na))
        rows["mc"].append(timed_mul(ctx["c"], ptr, nm, out, cnt))
        rows["mx"].append(timed_mul(ctx["x"], ptr, nm, out, cnt))
    res = {"runs": runs, "keys": na, "scalars": nm, "filter_MB": round(nwords * 8 / 1e6, 1), "geometry": {k: ctx[k].plan_geometry(na) for k in ("c", "x", "xe")}}
    for leg, n in (("c", na), ("x", na), ("xe", na), ("mc", nm), ("mx", nm)):
        res[leg] = {"event_M_per_s": [round(n / e / 1e6, 1) for e, _, _ in rows[leg]], "wall_M_per_s": [round(n / w / 1e6, 1) for _, w, _ in rows[leg]],
                    "event_median_M_per_s": round(statistics.median(n / e / 1e6 for e, _, _ in rows[leg]), 1),
                    "wall_median_M_per_s": round(statistics.median(n / w / 1e6 for _, w, _ in rows[leg]), 1), "hits": [h for _, _, h in rows[leg]]}
    res["x_over_c_event"] = round(res["x"]["event_median_M_per_s"] / res["c"]["event_median_M_per_s"], 3)
    res["xe_over_c_event"] = round(res["xe"]["event_median_M_per_s"] / res["c"]["event_median_M_per_s"], 3)
    res["mx_over_mc_event"] = round(res["mx"]["event_median_M_per_s"] / res["mc"]["event_median_M_per_s"], 3)
    res["coverage_x"] = ctx["x"].coverage()
    ctx["c"].lib.ecl_hip_free_host(ptr)
    for d in ctx.values():
        d.close()
    print(json.dumps(res))


def one_add(log2, endo):
    d = context(synth_bloom_words(7000003, 23, "a&(b|c)"), a33=False, pub=True, endo=endo)
    timed_add(d, START - (1 << 26), 1 << 26)
    ev, wall, total = timed_add(d, START, 1 << log2)
    print(json.dumps({"keys": 1 << log2, "endo": endo, "event_s": round(ev, 4), "wall_s": round(wall, 4), "event_M_per_s": round((1 << log2) / ev / 1e6, 1),
                      "hits": total, "geometry": d.plan_geometry(1 << log2)}))
    d.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "add":
        one_add(int(sys.argv[2]), len(sys.argv) > 3 and sys.argv[3] == "endo")
    elif len(sys.argv) > 1 and sys.argv[1] == "rates":
        a = [int(v) for v in sys.argv[2:]] + [None] * 4
        rates(a[0] or 3, a[1] or 32, a[2] or 26, a[3] or 7000003)
    else:
        sys.exit(__doc__)
