#!/usr/bin/env python3
"""The rates of `bsgs` on one GPU, in one process, profiler off - what the default beta rule waits for:
  baby24, baby28  the baby table: ECL_PUB | ECL_INSERT over 2^24 and 2^28 keys into a zeroed filter of one word per key (keys/s);
  giant           the giant walk: ECL_PUB | ECL_ORIGIN over 2^32 steps (ord_offs 30) against the beta = 28 filter (steps/s);
  copy            the beta = 28 filter (2 GB) from the insert context through host memory into the origin context (s);
  rescan          one window of 2^29 keys on an ordinary ECL_PUB context with a one-entry list (s).
Warm, `runs` alternating rounds, medians reported; kernel time from the library's HIP events, wall time beside it.  The target of the giant
walk is a key outside the range, so that every step is walked and nothing is resolved.

usage: bench_bsgs.py rates [runs = 3] [log2 giant steps = 32] [output = profiles/r10_bsgs.txt]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ecloop_amd import capi, engine  # noqa: E402

A = 0x100_0000_0000_0000_0000  # a range far above every baby step


def timed(d, start, n, **kw):
    ms0 = d.timing()[0]
    t0 = time.perf_counter()
    _, total = d.add_range(start, n, cap=1 << 16, **kw)
    wall = time.perf_counter() - t0
    return (d.timing()[0] - ms0) * 1e-3, wall, total


def rates(runs, lsteps, out_path):
    betas, nsteps = (24, 28), 1 << lsteps
    ins = {b: capi.Device(0, a33=False, pub=True, insert=True, ord_offs=1) for b in betas}
    giant = capi.Device(0, a33=False, pub=True, origin=True, ord_offs=30)
    scan = capi.Device(0, a33=False, pub=True)
    scan.set_lookahead(0)
    for d in list(ins.values()) + [giant, scan]:
        d.set_geometry(0, 1 << 20)  # four contexts side by side: 2^20 lanes each, so that none is cut back for want of memory
    rows = {k: [] for k in ("baby24", "baby28", "giant", "copy", "rescan")}
    plan = engine.bsgs_plan(A, A + nsteps * (2 << 28) - 1, 28)
    x, y, ok = scan.diag_mulg([A + nsteps * (2 << 28) + 12345])  # the target: a key behind the range
    origin = engine.bsgs_origin((x[0], y[0]))
    h5 = [(x[0] >> (32 * (7 - j))) & 0xFFFFFFFF for j in range(5)]
    one = np.zeros(1024, np.uint64)
    engine.blf_add_host(one, np.array([h5], np.uint32))
    scan.set_bloom(one)
    scan.set_list(np.array([h5], np.uint32))
    for r in range(runs + 1):  # round 0 warms: tables, buffers, code objects
        for b in betas:
            ins[b].set_bloom(np.zeros(1 << b, np.uint64))
            rows["baby%d" % b].append(timed(ins[b], 1, 1 << b))
        t0 = time.perf_counter()
        words = ins[28].get_bloom(1 << 28)
        giant.set_bloom(words)
        rows["copy"].append((None, time.perf_counter() - t0, 0))
        del words
        rows["giant"].append(timed(giant, plan["giant_start"], nsteps, origin=origin))
        rows["rescan"].append(timed(scan, A + r * (2 << 28), 2 << 28))
    res = {"runs": runs, "giant_steps": nsteps, "filter_MB": round((1 << 28) * 8 / 1e6, 1)}
    for leg, n in (("baby24", 1 << 24), ("baby28", 1 << 28), ("giant", nsteps)):
        got = rows[leg][1:]
        res[leg] = {"event_M_per_s": [round(n / e / 1e6, 1) for e, _, _ in got], "wall_M_per_s": [round(n / w / 1e6, 1) for _, w, _ in got],
                    "event_median_M_per_s": round(statistics.median(n / e / 1e6 for e, _, _ in got), 1),
                    "wall_median_M_per_s": round(statistics.median(n / w / 1e6 for _, w, _ in got), 1), "records": [t for _, _, t in got]}
    res["copy_s"] = {"wall": [round(w, 3) for _, w, _ in rows["copy"][1:]], "median": round(statistics.median(w for _, w, _ in rows["copy"][1:]), 3)}
    res["rescan_s"] = {"event": [round(e, 4) for e, _, _ in rows["rescan"][1:]], "wall": [round(w, 4) for _, w, _ in rows["rescan"][1:]],
                       "wall_median": round(statistics.median(w for _, w, _ in rows["rescan"][1:]), 4)}
    res["geometry"] = {"baby24": ins[24].plan_geometry(1 << 24), "baby28": ins[28].plan_geometry(1 << 28), "giant": giant.plan_geometry(nsteps)}
    res["coverage"] = {"baby28": ins[28].coverage(), "giant": giant.coverage()}
    for d in list(ins.values()) + [giant, scan]:
        d.close()
    text = json.dumps(res)
    print(text)
    if out_path:
        from ecloop_amd.build import source_sha256
        with open(out_path, "w") as f:
            f.write("tools/bench_bsgs.py rates %d %d - library sources sha256 %s\n%s\n" % (runs, lsteps, source_sha256(), json.dumps(res, indent=1)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rates":
        a = sys.argv[2:] + [None] * 3
        rates(int(a[0] or 3), int(a[1] or 32), a[2] or os.path.join(ROOT, "profiles", "r10_bsgs.txt"))
    else:
        sys.exit(__doc__)
