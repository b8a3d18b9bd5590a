#!/usr/bin/env python3
"""Prefix-search (`-p`) rate on one GPU, in one process, profiler off:
  p   ecl_hip_add_range with ECL_ADDR33 | ECL_PREFIX over 2^32 keys, the table of one long pattern (default 1BgGZ9tcN4);
  c   the same range with ECL_ADDR33 against a small `.blf` - the filter blf-gen sizes for 1000 entries (5392 bytes), with those many
      random hashes in it: the unchanged addr33 kernel of this build, its stage 1 one cached probe like the prefix kernel's bitmap load;
  o   `p` from an origin (ECL_ADDR33 | ECL_PREFIX | ECL_ORIGIN, the split-key search of DESIGN.md §7 (f12)): the same kernel, the same table and
      the same scalars, walked from the point Q = 0xdc2a04 G - the expected ratio o / p is 1 within the spread of the runs;
and for -a e, on the same range:
  e    ECL_ETH | ECL_PREFIX with the table of one long pattern (0xdeadbeefc0ffee): the yardstick of the two mask rows;
  m1   ECL_ETH | ECL_MASK with a table of one entry (0xdeadbeef*c0ffee);
  m16  ECL_ETH | ECL_MASK with a table of sixteen entries (0x<seven digits>*<three digits>, sixteen of them) - the most a table holds;
what is to be read off is m1 / e and m16 / e beside the run-to-run spread of e;
warm, `runs` alternating rounds, medians and their ratio reported.  Look-ahead off, 2^20 lanes per context (the half group stays automatic).

usage: bench_prefix.py rates [runs = 3] [log2 keys = 32] [pattern = 1BgGZ9tcN4]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ecloop_amd import capi, engine  # noqa: E402

START = 0x4000_0000_0000


def timed_add(d, start, n, origin=None):
    ms0 = d.timing()[0]
    t0 = time.perf_counter()
    recs, total = d.add_range(start, n, cap=1 << 16) if origin is None else d.add_range(start, n, cap=1 << 16, origin=origin)
    wall = time.perf_counter() - t0
    return (d.timing()[0] - ms0) * 1e-3, wall, total


def measure(ctx, origin, runs, n):
    """legs of one group: warm each, then `runs` alternating rounds -> leg -> [(event s, wall s, hits)]"""
    for leg, d in ctx.items():
        d.set_geometry(0, 1 << 20)
        timed_add(d, START - (1 << 28), 1 << 28, origin.get(leg))  # warm: tables, buffers, code objects
    rows = {leg: [] for leg in ctx}
    for r in range(runs):
        for leg in ctx:
            rows[leg].append(timed_add(ctx[leg], START + r * n, n, origin.get(leg)))
    return rows


def summary(rows, n):
    return {"event_M_per_s": [round(n / e / 1e6, 1) for e, _, _ in rows], "wall_M_per_s": [round(n / w / 1e6, 1) for _, w, _ in rows],
            "event_median_M_per_s": round(statistics.median(n / e / 1e6 for e, _, _ in rows), 1),
            "wall_median_M_per_s": round(statistics.median(n / w / 1e6 for _, w, _ in rows), 1), "hits": [h for _, _, h in rows]}


def spread(leg):
    return round(max(leg["event_M_per_s"]) / min(leg["event_M_per_s"]), 3)


def rates(runs, log2, pattern):
    n = 1 << log2
    table, _ = engine.prefix_ranges([pattern], True, False, False)
    words = np.zeros(engine.blf_size_words(1000), dtype=np.uint64)
    engine.blf_add_host(words, np.random.RandomState(1).randint(0, 1 << 32, size=(1000, 5), dtype=np.int64).astype(np.uint32))
    p = capi.Device(0, a33=True, prefix=True)
    p.set_prefixes(table)
    c = capi.Device(0, a33=True)
    c.set_bloom(words)
    c.set_lookahead(0)
    o = capi.Device(0, a33=True, prefix=True, origin=True)
    o.set_prefixes(table)
    xs, ys, ok = c.diag_mulg([0xDC2A04])
    ctx = {"p": p, "o": o, "c": c}
    rows = measure(ctx, {"o": (xs[0], ys[0])}, runs, n)
    res = {"runs": runs, "keys": n, "pattern": pattern, "ranges": len(table), "blf_bytes": len(words) * 8,
           "geometry": {k: ctx[k].plan_geometry(n) for k in ctx}}
    for leg in ctx:
        res[leg] = summary(rows[leg], n)
    res["p_over_c_event"] = round(res["p"]["event_median_M_per_s"] / res["c"]["event_median_M_per_s"], 3)
    res["o_over_p_event"] = round(res["o"]["event_median_M_per_s"] / res["p"]["event_median_M_per_s"], 3)
    res["p_spread_event"], res["o_spread_event"] = spread(res["p"]), spread(res["o"])
    res["coverage_p"] = p.coverage()
    res["coverage_o"] = o.coverage()
    for d in ctx.values():
        d.close()
    # the -a e rows, a group of their own (the first group's contexts and their walk buffers are gone)
    e = capi.Device(0, a33=False, eth=True, prefix=True)
    e.set_prefixes(engine.prefix_ranges(["0xdeadbeefc0ffee"], False, False, True)[0])
    m1 = capi.Device(0, a33=False, eth=True, mask=True)
    m1.set_masks(engine.mask_table(["0xdeadbeef*c0ffee"])[0])
    m16 = capi.Device(0, a33=False, eth=True, mask=True)
    m16.set_masks(engine.mask_table(["0x%07x*%03x" % (0xDEAD000 + 7 * i, 0xBE0 + i) for i in range(16)])[0])
    ctx = {"e": e, "m1": m1, "m16": m16}
    rows = measure(ctx, {}, runs, n)
    res["geometry"].update({k: ctx[k].plan_geometry(n) for k in ctx})
    for leg in ctx:
        res[leg] = summary(rows[leg], n)
    for leg in ("m1", "m16"):
        res[leg + "_over_e_event"] = round(res[leg]["event_median_M_per_s"] / res["e"]["event_median_M_per_s"], 3)
        res["coverage_" + leg] = ctx[leg].coverage()
    res["e_spread_event"] = spread(res["e"])
    res["mask_entries"] = {"m1": 1, "m16": 16}
    for d in ctx.values():
        d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rates":
        a = sys.argv[2:] + [None] * 3
        rates(int(a[0] or 3), int(a[1] or 32), a[2] or "1BgGZ9tcN4")
    else:
        sys.exit(__doc__)
