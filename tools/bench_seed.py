#!/usr/bin/env python3
"""`seed` rates on one GPU, profiler off: ecl_hip_mul_batch_raw on a Device(bip39=True), -a c, a small filter.
  rates  calls of 2^log2 phrases from page-locked text and table - 12-word phrases with reuse = 0, 24-word phrases with reuse = 0 (an
         HMAC key longer than a block: hashed first), and a reuse = 1 call of the same size with BIP44's path - a warm call of each, then
         `runs` alternating rounds; the device's own time (ecl_hip_get_mul_timing: the call's events) and the wall time, medians.
         Beside them the issue-cycle floor of k_bip39_master's iteration loop from the assembly the build keeps (tools/isa_mix.py --seed)
         and the measured fraction of it.

usage: bench_seed.py rates [runs = 3] [log2 phrases = 20]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ecloop_amd import capi, engine  # noqa: E402

WORDS = ["abandon", "ability", "able", "about", "above", "absent", "absorb", "abstract", "absurd", "abuse", "access", "accident", "zone", "zoo", "wrong", "year"]
BIP44 = [44 | 1 << 31, 1 << 31, 1 << 31, 0, 0]
RECORD_ROOM = 160


def phrase_text(n, nwords, seed):
    """n distinct phrases of nwords words behind the record's slot -> (uint8 text, table[1:])"""
    rnd = np.random.RandomState(seed)
    pick = rnd.randint(0, len(WORDS), size=(n, nwords))
    lines = [" ".join(WORDS[j] for j in row) + " %d" % i for i, row in enumerate(pick)]
    ln = np.array([len(l) for l in lines], dtype=np.uint64)
    starts = RECORD_ROOM + np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    text = np.concatenate([np.zeros(RECORD_ROOM, np.uint8), np.frombuffer("".join(lines).encode(), dtype=np.uint8)])
    return text, starts | (ln << np.uint64(32))


class Call:
    """page-locked text and table of one input; the record is rewritten in its slot for every call"""

    def __init__(self, d, text, table):
        self.d, self.nbytes, self.n = d, len(text), len(table) + 1
        self.ptext, self.ptable = d.lib.ecl_hip_alloc_host(len(text) + 16), d.lib.ecl_hip_alloc_host(self.n * 8)
        self.text = np.ctypeslib.as_array(C.cast(self.ptext, C.POINTER(C.c_uint8)), shape=(len(text),))
        self.table = np.ctypeslib.as_array(C.cast(self.ptable, C.POINTER(C.c_uint64)), shape=(self.n,))
        self.text[:], self.table[1:] = text, table
        self.out = np.zeros(1 << 12, dtype=capi.FOUND_DTYPE)

    def run(self, path, reuse):
        rec = capi.Device.seed_record(path, b"", reuse)
        self.text[: len(rec)] = np.frombuffer(rec, dtype=np.uint8)
        self.table[0] = len(rec) << 32
        ms0, cnt = self.d.mul_timing()[0], C.c_uint32()
        t0 = time.perf_counter()
        rc = self.d.lib.ecl_hip_mul_batch_raw(self.d.h, self.ptext, self.nbytes, self.ptable, self.n, self.out.ctypes.data, len(self.out), C.byref(cnt))
        wall = time.perf_counter() - t0
        assert rc == 0, (rc, self.d.lib.ecl_hip_last_error(self.d.h))
        return (self.d.mul_timing()[0] - ms0) * 1e-3, wall

    def free(self):
        self.d.lib.ecl_hip_free_host(self.ptext), self.d.lib.ecl_hip_free_host(self.ptable)


def rates(runs, log2):
    import isa_mix
    n = 1 << log2
    words = np.zeros(engine.blf_size_words(1000), dtype=np.uint64)
    engine.blf_add_host(words, np.random.RandomState(1).randint(0, 1 << 32, size=(1000, 5), dtype=np.int64).astype(np.uint32))
    d = capi.Device(0, a33=True, bip39=True)
    d.set_bloom(words)
    calls = {12: Call(d, *phrase_text(n, 12, 12)), 24: Call(d, *phrase_text(n, 24, 24))}
    legs = {"12 words, reuse = 0": lambda: calls[12].run(BIP44, False), "24 words, reuse = 0": lambda: calls[24].run(BIP44, False),
            "reuse = 1, m/44'/0'/0'/0/1": lambda: calls[24].run(BIP44[:4] + [1], True)}
    rows = {k: [] for k in legs}
    for k, f in legs.items():  # warm: tables, buffers
        f()
    for _ in range(runs):
        for k, f in legs.items():
            rows[k].append(f())
    res = {"phrases_per_call": n, "runs": runs, "coverage": d.coverage()}
    for k, v in rows.items():
        res[k] = {"event_M_per_s": [round(n / e / 1e6, 3) for e, _ in v], "wall_M_per_s": [round(n / w / 1e6, 3) for _, w in v],
                  "event_median_M_per_s": round(statistics.median(n / e / 1e6 for e, _ in v), 3), "wall_median_M_per_s": round(statistics.median(n / w / 1e6 for _, w in v), 3)}
    try:
        it = isa_mix.analyse_seed()["master"]["iteration_loop"]
        res["floor"] = {"per_iteration": it["per_iteration"], "clocks_per_iteration": it["clocks_per_iteration"], "floor_M_phrases_per_s": round(it["floor_phrases_per_s"] / 1e6, 3)}
        for k in list(legs)[:2]:
            res[k]["fraction_of_floor"] = round(res[k]["event_median_M_per_s"] * 1e6 / it["floor_phrases_per_s"], 3)
    except Exception as e:  # no kept assembly (a library that was not built here)
        res["floor"] = {"unavailable": str(e)}
    for c in calls.values():
        c.free()
    d.close()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rates":
        a = sys.argv[2:] + [None] * 2
        rates(int(a[0] or 3), int(a[1] or 20))
    else:
        print(__doc__)
