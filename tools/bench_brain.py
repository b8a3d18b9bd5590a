#!/usr/bin/env python3
"""`brain` rates on one GPU, profiler off: ecl_hip_mul_batch_raw on a Device(gen=True), -a c, a small filter.
  rates  calls of 2^log2 candidates through the ABI for three templates - an 8-byte mask (?l?l?l?l?l?l?d?d), a 12-byte mask
         (pass?l?l?l?l?d?d?d?d) and two dictionaries of 4096 words of 3 ... 10 bytes with a space between - under sha256 and keccak.
         The yardstick, in the same process on the same box: ecl_hip_mul_batch_raw over the SAME 2^log2 lines, sent as text and line
         table from page-locked memory to a context without the flag.  A warm call of each leg, then `runs` rounds that alternate the
         legs.  Both legs are timed as tools/bench_kdf.py times its calls: the device's own time (ecl_hip_get_mul_timing: the
         call's events, the figure profiles/r16_kdf.txt quotes) and the host's wall time per call - all values and the medians of both, and
         the yardstick's own spread (max / min) as the margin.

usage: bench_brain.py rates [runs = 5] [log2 candidates = 24]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ecloop_amd import capi, engine  # noqa: E402


def dictionary(n, seed):
    rnd = np.random.RandomState(seed)
    return [bytes(rnd.randint(97, 123, size=rnd.randint(3, 11)).astype(np.uint8)) for _ in range(n)]


def templates():
    words = dictionary(4096, 7)
    return {"mask 8": engine.parse_mask("?l?l?l?l?l?l?d?d"), "mask 12": engine.parse_mask("pass?l?l?l?l?d?d?d?d"), "two dictionaries": [words, [b" "], dictionary(4096, 8)]}


def lines_of(positions, n):
    """candidates 0 ... n - 1 as (uint8 text, line table), with numpy: the digits by division, the bytes column by column"""
    idx = np.arange(n, dtype=np.uint64)
    digits = []
    for p in reversed(positions):
        digits.append((idx % np.uint64(len(p))).astype(np.int64))
        idx //= np.uint64(len(p))
    digits.reverse()
    lens = [np.array([len(a) for a in p], dtype=np.int64)[d] for p, d in zip(positions, digits)]
    total = np.sum(lens, axis=0)
    starts = np.concatenate([[0], np.cumsum(total)[:-1]])
    text = np.zeros(int(total.sum()), dtype=np.uint8)
    at = starts.copy()
    for p, d, l in zip(positions, digits, lens):
        width = max(len(a) for a in p)
        padded = np.zeros((len(p), max(width, 1)), dtype=np.uint8)
        for i, a in enumerate(p):
            padded[i, : len(a)] = np.frombuffer(a, dtype=np.uint8)
        for k in range(width):
            live = l > k
            text[at[live] + k] = padded[d[live], k]
        at += l
    return text, starts.astype(np.uint64) | (total.astype(np.uint64) << np.uint64(32))


class Sent:
    """the yardstick's input in page-locked memory"""

    def __init__(self, d, text, table):
        self.d, self.nbytes, self.n = d, len(text), len(table)
        self.ptext, self.ptable = d.lib.ecl_hip_alloc_host(len(text) + 16), d.lib.ecl_hip_alloc_host(self.n * 8)
        np.ctypeslib.as_array(C.cast(self.ptext, C.POINTER(C.c_uint8)), shape=(len(text),))[:] = text
        np.ctypeslib.as_array(C.cast(self.ptable, C.POINTER(C.c_uint64)), shape=(self.n,))[:] = table
        self.out = np.zeros(1 << 12, dtype=capi.FOUND_DTYPE)

    def run(self):
        ms0, cnt = self.d.mul_timing()[0], C.c_uint32()
        t0 = time.perf_counter()
        rc = self.d.lib.ecl_hip_mul_batch_raw(self.d.h, self.ptext, self.nbytes, self.ptable, self.n, self.out.ctypes.data, len(self.out), C.byref(cnt))
        wall = time.perf_counter() - t0
        assert rc == 0, (rc, self.d.lib.ecl_hip_last_error(self.d.h))
        return (self.d.mul_timing()[0] - ms0) * 1e-3, wall, cnt.value

    def free(self):
        self.d.lib.ecl_hip_free_host(self.ptext), self.d.lib.ecl_hip_free_host(self.ptable)


class Generated:
    def __init__(self, d, positions, n):
        self.d, self.n = d, n
        self.blob = np.frombuffer(engine.brain_table(positions), dtype=np.uint8).copy()
        self.first = np.zeros(1, dtype=np.uint64)
        self.out = np.zeros(1 << 12, dtype=capi.FOUND_DTYPE)

    def run(self):
        ms0, cnt = self.d.mul_timing()[0], C.c_uint32()
        t0 = time.perf_counter()
        rc = self.d.lib.ecl_hip_mul_batch_raw(self.d.h, self.blob.ctypes.data, len(self.blob), self.first.ctypes.data, self.n, self.out.ctypes.data, len(self.out), C.byref(cnt))
        wall = time.perf_counter() - t0
        assert rc == 0, (rc, self.d.lib.ecl_hip_last_error(self.d.h))
        return (self.d.mul_timing()[0] - ms0) * 1e-3, wall, cnt.value


def rates(runs, log2):
    n = 1 << log2
    words = np.zeros(engine.blf_size_words(1000), dtype=np.uint64)
    engine.blf_add_host(words, np.random.RandomState(1).randint(0, 1 << 32, size=(1000, 5), dtype=np.int64).astype(np.uint32))
    res = {"candidates_per_call": n, "runs": runs}
    for kdf in ("sha256", "keccak"):
        gen, plain = capi.Device(0, a33=True, kdf=None if kdf == "sha256" else kdf, gen=True), capi.Device(0, a33=True, kdf=None if kdf == "sha256" else kdf)
        gen.set_bloom(words), plain.set_bloom(words)
        for name, positions in templates().items():
            legs = {"generated": Generated(gen, positions, n), "sent": Sent(plain, *lines_of(positions, n))}
            hits = {k: leg.run()[2] for k, leg in legs.items()}  # warm: tables, buffers, the template's upload
            assert hits["generated"] == hits["sent"], hits  # the same candidates pass the filter
            rows = {k: [] for k in legs}
            for _ in range(runs):
                for k, leg in legs.items():
                    rows[k].append(leg.run()[:2])
            legs["sent"].free()
            ev = {k: [e for e, _ in v] for k, v in rows.items()}
            wl = {k: [w for _, w in v] for k, v in rows.items()}
            r = {k: {"event_M_per_s": [round(n / e / 1e6, 1) for e in ev[k]], "wall_M_per_s": [round(n / w / 1e6, 1) for w in wl[k]],
                     "event_median_M_per_s": round(n / statistics.median(ev[k]) / 1e6, 1), "wall_median_M_per_s": round(n / statistics.median(wl[k]) / 1e6, 1)} for k in rows}
            r["sent"]["event_spread"], r["sent"]["wall_spread"] = round(max(ev["sent"]) / min(ev["sent"]), 4), round(max(wl["sent"]) / min(wl["sent"]), 4)
            r["generated_over_sent"] = {"event": round(statistics.median(ev["sent"]) / statistics.median(ev["generated"]), 4),
                                        "wall": round(statistics.median(wl["sent"]) / statistics.median(wl["generated"]), 4)}
            r["filter_hits"] = hits["generated"]
            res["%s, %s" % (kdf, name)] = r
        res["coverage, %s" % kdf] = {"generated": gen.coverage(), "sent": plain.coverage()}
        gen.close(), plain.close()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rates":
        a = sys.argv[2:] + [None] * 2
        rates(int(a[0] or 5), int(a[1] or 24))
    else:
        print(__doc__)
