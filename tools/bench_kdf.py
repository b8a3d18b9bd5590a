#!/usr/bin/env python3
"""`mul -raw -kdf` rates on one GPU, profiler off.  Input: tools/gen_phrases.c lines (8..24 characters).
  abi   ecl_hip_mul_batch_raw on calls of 2^24 lines (camp2: 2^20) from page-locked text and table, -a c, a small .blf: per KDF a warm
        call, then `runs` alternating rounds; the device's own time (ecl_hip_get_mul_timing) and the wall time, medians;
  cli   the host program, `mul -raw -kdf <name> -a c -q` with a file on stdin, at two sizes (2^24 and 2^27 lines; camp2 2^20 and 2^22):
        the wall time of each whole run, and the rate of the lines the longer run has more - the bring-up (contexts, self-test, tables:
        half a second) drops out of the difference;
  camp2 is also given as permutations/s (x 2031) beside the issue-cycle floor of its loop, from the loop's static instruction mix in the
        assembly the build keeps (tools/isa_mix.py) on 256 CUs x 4 SIMDs at the nominal 2.4 GHz: with the classes priced as bench.py
        prices them for the other kernels (add / logic / v_bitop3_b32 at their long-run 2.4 SIMD cycles per wave64 instruction, rotates
        and the rest at 4.1: profiles/ubench_r03.txt), and with every instruction at 4 cycles;
  ab    (with a second library) sha256 alone, in child processes that alternate between that library and this build's: the kernel of
        sha256 is unchanged, so the two medians must lie within the spread of either.

usage: bench_kdf.py rates [runs = 3] [log2 lines = 24] [log2 camp2 lines = 20] [other libecloop_hip.so] [log2 lines of the long cli run = 27]
       bench_kdf.py sha256 <lines file> <runs>      (the child of `ab`: the library is $ECLOOP_HIP_LIB)"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ecloop_amd import capi, engine  # noqa: E402

KDFS = ("sha256", "keccak", "sha3", "camp2")
CAMP2_LOOP = "_Z19k_raw_scalars_camp2PKjjjPKmjPjS3_"
SIMD_CYCLES = 256 * 4 * 2.4e9  # SIMD cycles per second
CYCLES_FAST, CYCLES_OTHER = 2.4, 4.1  # per wave64 instruction, by class (tools/isa_mix.py: classify)


def phrases(n, path):
    """n lines of tools/gen_phrases.c (the generator is built in a directory of its own: /dev/shm may not run programs)"""
    with tempfile.TemporaryDirectory(prefix="genphrases") as d:
        exe = os.path.join(d, "gen_phrases")
        subprocess.run(["gcc", "-O2", "-pthread", os.path.join(ROOT, "tools", "gen_phrases.c"), "-o", exe], check=True)
        subprocess.run([exe, str(n), "11", path, "16"], check=True, stdout=subprocess.DEVNULL)


def line_table(text):
    """uint8 text of '\\n'-terminated lines -> offset | length << 32"""
    ends = np.flatnonzero(text == 10).astype(np.uint64)
    starts = np.concatenate([[0], ends[:-1] + 1]).astype(np.uint64)
    return starts | ((ends - starts) << np.uint64(32))


class Pinned:
    """page-locked copies of a text and its table (ecl_hip_alloc_host): the call reads them by DMA"""

    def __init__(self, lib, text, table):
        self.lib, self.nbytes, self.n = lib, len(text), len(table)
        self.ptext, self.ptable = lib.ecl_hip_alloc_host(len(text) + 16), lib.ecl_hip_alloc_host(len(table) * 8)
        np.ctypeslib.as_array(C.cast(self.ptext, C.POINTER(C.c_uint8)), shape=(len(text),))[:] = text
        np.ctypeslib.as_array(C.cast(self.ptable, C.POINTER(C.c_uint64)), shape=(len(table),))[:] = table

    def free(self):
        self.lib.ecl_hip_free_host(self.ptext), self.lib.ecl_hip_free_host(self.ptable)


def timed_raw(d, pin, out):
    ms0, cnt = d.mul_timing()[0], C.c_uint32()
    t0 = time.perf_counter()
    rc = d.lib.ecl_hip_mul_batch_raw(d.h, pin.ptext, pin.nbytes, pin.ptable, pin.n, out.ctypes.data, len(out), C.byref(cnt))
    wall = time.perf_counter() - t0
    assert rc == 0, (rc, d.lib.ecl_hip_last_error(d.h))
    return (d.mul_timing()[0] - ms0) * 1e-3, wall, cnt.value


def small_filter():
    words = np.zeros(engine.blf_size_words(1000), dtype=np.uint64)
    engine.blf_add_host(words, np.random.RandomState(1).randint(0, 1 << 32, size=(1000, 5), dtype=np.int64).astype(np.uint32))
    return words


def summary(rows, n):
    return {"event_M_per_s": [round(n / e / 1e6, 2) for e, _, _ in rows], "wall_M_per_s": [round(n / w / 1e6, 2) for _, w, _ in rows],
            "event_median_M_per_s": round(statistics.median(n / e / 1e6 for e, _, _ in rows), 2),
            "wall_median_M_per_s": round(statistics.median(n / w / 1e6 for _, w, _ in rows), 2), "hits": [h for _, _, h in rows]}


def read_lines(path):
    text = np.fromfile(path, dtype=np.uint8)
    return text, line_table(text)


def sha256_child(path, runs):
    text, table = read_lines(path)
    d = capi.Device(0, a33=True)
    d.set_bloom(small_filter())
    pin, out = Pinned(d.lib, text, table), np.zeros(1 << 16, dtype=capi.FOUND_DTYPE)
    timed_raw(d, pin, out)
    rows = [timed_raw(d, pin, out) for _ in range(runs)]
    print(json.dumps(dict(summary(rows, len(table)), lib=capi.LIB_PATH, lines=len(table), coverage=d.coverage())))
    pin.free(), d.close()


def camp2_floor():
    try:
        import isa_mix
        loops = isa_mix.analyse(isa_mix.ASM, CAMP2_LOOP)["loops"]
        loop = min((l for l in loops if l["vmem"] == 0), key=lambda l: l["valu"])  # the 2030-trip loop: one permutation, no memory instruction
        perms = SIMD_CYCLES * 64 / (loop["fast"] * CYCLES_FAST + (loop["valu"] - loop["fast"]) * CYCLES_OTHER)
        single = SIMD_CYCLES * 64 / (loop["valu"] * 4.0)
        return {"loop_valu": loop["valu"], "loop_fast": loop["fast"], "loop_other": loop["other"], "loop_scratch": loop["scratch"],
                "cycles_per_class": {"fast": CYCLES_FAST, "other": CYCLES_OTHER},
                "floor_G_permutations_per_s": round(perms / 1e9, 3), "floor_M_lines_per_s": round(perms / 2031 / 1e6, 3),
                "every_instruction_at_4_cycles_G_permutations_per_s": round(single / 1e9, 3)}
    except Exception as e:  # no kept assembly (a library that was not built here)
        return {"unavailable": str(e)}


def rates(runs, log2, log2_camp2, other, log2_long):
    tmp = tempfile.mkdtemp(prefix="benchkdf", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    big, small = os.path.join(tmp, "lines.txt"), os.path.join(tmp, "lines_camp2.txt")
    long, long_camp2 = os.path.join(tmp, "lines_long.txt"), os.path.join(tmp, "lines_camp2_long.txt")
    phrases(1 << log2, big), phrases(1 << log2_camp2, small), phrases(1 << log2_long, long), phrases(4 << log2_camp2, long_camp2)
    res = {"runs": runs, "lines": 1 << log2, "camp2_lines": 1 << log2_camp2, "bytes": os.path.getsize(big)}
    # ---- through the ABI
    words = small_filter()
    out = np.zeros(1 << 16, dtype=capi.FOUND_DTYPE)
    ctx = {k: capi.Device(0, a33=True, kdf=None if k == "sha256" else k) for k in KDFS}
    pins = {}
    for path in (big, small):
        text, table = read_lines(path)
        pins[path] = Pinned(ctx["sha256"].lib, text, table)
    rows = {k: [] for k in KDFS}
    for k, d in ctx.items():
        d.set_bloom(words)
        timed_raw(d, pins[small if k == "camp2" else big], out)  # warm: table, buffers, code objects
    for _ in range(runs):
        for k, d in ctx.items():
            rows[k].append(timed_raw(d, pins[small if k == "camp2" else big], out))
    res["abi"] = {k: summary(rows[k], pins[small if k == "camp2" else big].n) for k in KDFS}
    res["abi"]["coverage"] = {k: ctx[k].coverage() for k in KDFS}
    for d in ctx.values():
        d.close()
    for p in pins.values():
        p.free()
    floor = camp2_floor()
    got = res["abi"]["camp2"]["event_median_M_per_s"]
    res["camp2"] = dict(floor, M_lines_per_s=got, G_permutations_per_s=round(got * 2031 / 1e3, 3))
    if "floor_M_lines_per_s" in floor:
        res["camp2"]["fraction_of_floor"] = round(got / floor["floor_M_lines_per_s"], 3)
    # ---- through the host program
    cli = os.path.join(ROOT, "ecloop_amd", "host", "ecloop-hip")
    blf = os.path.join(tmp, "small.blf")
    engine.blf_save(blf, words)
    res["cli"] = {}
    def run_cli(k, path):
        t0 = time.perf_counter()
        subprocess.run([cli, "mul", "-raw", "-kdf", k, "-f", blf, "-a", "c", "-q", "-o", os.path.join(tmp, "found.txt")], stdin=open(path, "rb"),
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=600)
        return time.perf_counter() - t0
    for k in KDFS:
        (p1, n1), (p2, n2) = ((small, 1 << log2_camp2), (long_camp2, 4 << log2_camp2)) if k == "camp2" else ((big, 1 << log2), (long, 1 << log2_long))
        w1, w2 = [run_cli(k, p1) for _ in range(runs)], [run_cli(k, p2) for _ in range(runs)]
        res["cli"][k] = {"lines": [n1, n2], "wall_s": [[round(w, 3) for w in w1], [round(w, 3) for w in w2]],
                         "whole_run_median_M_per_s": round(n2 / statistics.median(w2) / 1e6, 2),
                         "marginal_M_per_s": round((n2 - n1) / (statistics.median(w2) - statistics.median(w1)) / 1e6, 2)}
    # ---- sha256 against another build of the library, alternating child processes
    if other:
        ab = {"other": [], "this": []}
        for _ in range(runs):
            for leg, lib in (("other", other), ("this", capi.LIB_PATH)):
                pr = subprocess.run([sys.executable, os.path.abspath(__file__), "sha256", big, "3"], env=dict(os.environ, ECLOOP_HIP_LIB=lib), capture_output=True,
                                    text=True, check=True, timeout=600)
                ab[leg].append(json.loads(pr.stdout.strip().splitlines()[-1])["event_median_M_per_s"])
        res["sha256_ab"] = {leg: {"event_median_M_per_s_of_each_process": v, "median": statistics.median(v), "spread": round(max(v) / min(v), 4)} for leg, v in ab.items()}
        res["sha256_ab"]["this_over_other"] = round(res["sha256_ab"]["this"]["median"] / res["sha256_ab"]["other"]["median"], 4)
    for f in os.listdir(tmp):
        os.unlink(os.path.join(tmp, f))
    os.rmdir(tmp)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rates":
        a = sys.argv[2:] + [None] * 5
        rates(int(a[0] or 3), int(a[1] or 24), int(a[2] or 20), a[3] or None, int(a[4] or 27))
    elif len(sys.argv) > 3 and sys.argv[1] == "sha256":
        sha256_child(sys.argv[2], int(sys.argv[3]))
    else:
        sys.exit(__doc__)
