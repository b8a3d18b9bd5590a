#!/usr/bin/env python3
"""The rates of `kangaroo` on one GPU, in one process, profiler off - where the numbers that section marks "not
measured" come from:
  jumps/s of the herd walk (ECL_PUB | ECL_HERD) for a few herd sizes H and distinguished-point widths dp on a fixed range of 2^96 keys,
    the target a key outside the range, so that every jump is walked and nothing is resolved; dp = 32 beside a small dp gives the
    overhead of reporting distinguished points;
  the set-up of a herd (ms per build);
  the crossover against `bsgs`: with its giant rate g (steps/s, from tools/bench_bsgs.py's output if given, else not computed), bsgs walks
    W / 2^31 steps at its largest baby table and kangaroo expects 2 sqrt(W) + H 2^dp jumps at the best rate j measured here: the width W at
    which the two times are equal.
Warm, `runs` rounds, medians reported; kernel time from the library's HIP events, wall time beside it.

usage: bench_kangaroo.py rates [runs = 3] [log2 jumps per call = 30] [bsgs giant steps/s] [output = profiles/r11_kangaroo.txt]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ecloop_amd import capi, engine  # noqa: E402

A = 0x100_0000_0000_0000_0000_0000_0000
WBITS = 96


def rates(runs, ljumps, giant_rate, out_path):
    probe = capi.Device(0, a33=False, pub=True)
    x, y, _ = probe.diag_mulg([A + (1 << WBITS) + 12345])
    probe.close()
    q = (x[0], y[0])
    res = {"runs": runs, "jumps_per_call": 1 << ljumps, "range_bits": WBITS, "legs": {}}
    best = 0.0
    for hl in (16, 20, 22, 24):
        for dp in (8, 32):
            plan = engine.kangaroo_plan(A, A + (1 << WBITS) - 1, hl, dp)
            block = (plan["base"], q, 1, hl, plan["jb"], plan["sb"])
            d = capi.Device(0, a33=False, pub=True, herd=True, ord_offs=dp)
            rows = []
            for _ in range(runs + 1):  # round 0 builds the herd and warms
                ms0 = d.timing()[0]
                t0 = time.perf_counter()
                _, total = d.add_range(None, 1 << ljumps, cap=1 << 16, herd=block)
                rows.append(((d.timing()[0] - ms0) * 1e-3, time.perf_counter() - t0, total))
            setup_ms, setups = d.setup_timing()
            cov = d.coverage()
            d.close()
            got = rows[1:]
            ev = statistics.median((1 << ljumps) / e / 1e6 for e, _, _ in got)
            res["legs"]["H=2^%d dp=%d" % (hl, dp)] = {
                "event_median_M_jumps_per_s": round(ev, 1), "wall_median_M_jumps_per_s": round(statistics.median((1 << ljumps) / w / 1e6 for _, w, _ in got), 1),
                "event_M_jumps_per_s": [round((1 << ljumps) / e / 1e6, 1) for e, _, _ in got], "records": [t for _, _, t in got],
                "setup_ms": round(setup_ms, 2), "setups": setups, "coverage": cov}
            best = max(best, ev * 1e6)
    if giant_rate:
        # bsgs: W / 2^31 giant steps at g steps/s; kangaroo: about 2 sqrt(W) jumps at j jumps/s -> equal at sqrt(W) = 2^32 g / j
        res["crossover_bits_against_bsgs"] = round(2 * (32 + __import__("math").log2(giant_rate / best)), 1)
    text = json.dumps(res)
    print(text)
    if out_path:
        from ecloop_amd.build import source_sha256
        with open(out_path, "w") as f:
            f.write("tools/bench_kangaroo.py rates %d %d - library sources sha256 %s\n%s\n" % (runs, ljumps, source_sha256(), json.dumps(res, indent=1)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rates":
        a = sys.argv[2:] + [None] * 4
        rates(int(a[0] or 3), int(a[1] or 30), float(a[2]) if a[2] else None, a[3] or os.path.join(ROOT, "profiles", "r11_kangaroo.txt"))
    else:
        sys.exit(__doc__)
