"""`kangaroo` (Pollard's lambda search for a known public key; ECL_HERD) without a GPU: the plan header the library and the CLI run
(host/kangaroo_plan.h) and the step arithmetic of the herd kernel (csrc/herd_kernel.h), compiled for the host (csrc/tools/kangaroo_host.cpp),
against tests/kangaroo_ref.py, a pure-Python restatement over the oracle's points; the pins of the C ABI header and the binding; the CLI's
refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kangaroo_ref as ref
import orc
from support import ROOT, cli, host_lib, host_program, int_of, run_program

P, N = orc.P, orc.N
M64 = (1 << 64) - 1


def limbs(v, n=4):
    return [(v >> (64 * i)) & M64 for i in range(n)]


def arr(v, n=4):
    return np.array(limbs(v, n), np.uint64)


def words8(v):
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)], np.uint32)


@pytest.fixture(scope="module")
def K(tmp_path_factory):
    lib = host_lib(tmp_path_factory, "kangaroo_host.cpp")
    V = C.c_void_p
    lib.kh_table.argtypes = [C.c_uint64, C.c_uint, V]
    lib.kh_table.restype = None
    lib.kh_offsets.argtypes = [C.c_uint64, C.c_uint, C.c_uint, C.c_uint32, V]
    lib.kh_offsets.restype = None
    lib.kh_new.argtypes = [V]
    lib.kh_new.restype = V
    lib.kh_free.argtypes = [V]
    lib.kh_free.restype = None
    lib.kh_run.argtypes = [V, C.c_uint32, C.c_uint32, V, C.c_uint32]
    lib.kh_run.restype = C.c_uint32
    lib.kh_get.argtypes = [V, C.c_uint32, V, V, V]
    lib.kh_get.restype = None
    lib.kh_set.argtypes = [V, C.c_uint32, V, V]
    lib.kh_set.restype = None
    lib.kh_zero_factors.argtypes = [V]
    lib.kh_zero_factors.restype = C.c_uint64
    lib.kh_overflow.argtypes = [V]
    lib.kh_overflow.restype = C.c_uint32
    lib.kh_is_dp.argtypes = [V, C.c_uint32]
    lib.kh_is_dp.restype = C.c_int
    lib.kh_plan.argtypes = [V, V, C.c_int, C.c_int, V]
    lib.kh_give_up.argtypes = [V, V, C.c_int, C.c_int, C.c_uint32, V]
    lib.kh_candidates.argtypes = [V] * 5
    lib.kh_candidates.restype = None
    return lib


def block(base, q, seed, herd_log2, jb, sb):
    return np.array(limbs(base) + limbs(q[0]) + limbs(q[1]) + [seed & M64, herd_log2, jb, sb], np.uint64)


class HostHerd:
    """the herd of kangaroo_host.cpp: the C step arithmetic of the kernel"""

    def __init__(self, K, base, q, seed, herd_log2, jb, sb):
        self.K, self.H = K, 1 << herd_log2
        self.blk = block(base, q, seed, herd_log2, jb, sb)
        self.h = K.kh_new(self.blk.ctypes.data)
        assert self.h

    def run(self, steps, dp):
        cap = steps * self.H
        recs = np.zeros((cap, 8), np.uint32)
        n = self.K.kh_run(self.h, steps, dp, recs.ctypes.data, cap)
        assert n <= cap
        return [(int(r[0]) | int(r[1]) << 32, tuple(int(v) for v in r[2:7]), int(r[7]) & 255, int(r[7]) >> 8) for r in recs[:n]]

    def get(self, i):
        x, y, d = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(4, np.uint32)
        self.K.kh_get(self.h, i, x.ctypes.data, y.ctypes.data, d.ctypes.data)
        return tuple(sum(int(w) << (32 * j) for j, w in enumerate(v)) for v in (x, y, d))

    def set(self, i, pt):
        x, y = words8(pt[0]), words8(pt[1])
        self.K.kh_set(self.h, i, x.ctypes.data, y.ctypes.data)

    def close(self):
        self.K.kh_free(self.h)


CASES = [(1, 3, 10, 12), (1, 0, 4, 1), (7, 9, 20, 30), (7, 0xFFFFFFFFFFFFFFFF, 63, 64), (6, 1, 120, 124), (5, 77, 64, 65), (8, 5, 22, 32)]


def test_stream_table_and_offsets(K):
    """the distances (all distinct, 1 ... 2^(jb + 1)) and the offsets (below 2^sb) of the C header equal the yardstick's, draw for draw"""
    for herd_log2, seed, jb, sb in CASES:
        s, r = ref.distances_and_offsets(seed, herd_log2, jb, sb)
        got = np.zeros(64, np.uint64)
        K.kh_table(seed, jb, got.ctypes.data)
        assert [int(got[2 * j]) | int(got[2 * j + 1]) << 64 for j in range(32)] == s
        assert len(set(s)) == 32 and all(1 <= v <= 1 << (jb + 1) for v in s)
        off = np.zeros(2 << herd_log2, np.uint64)
        K.kh_offsets(seed, jb, sb, 1 << herd_log2, off.ctypes.data)
        assert [int(off[2 * i]) | int(off[2 * i + 1]) << 64 for i in range(1 << herd_log2)] == r and all(v < 1 << sb for v in r)
    # jb = 4 leaves exactly 32 values: the table is a permutation of 1 ... 32, whatever was drawn again on the way
    got = np.zeros(64, np.uint64)
    K.kh_table(11, 4, got.ctypes.data)
    assert sorted(int(v) for v in got[0::2]) == list(range(1, 33)) == sorted(ref.table(ref.Stream(11), 4)) and not got[1::2].any()
    assert [int(v) for v in got[0::2]] == ref.table(ref.Stream(11), 4)


@pytest.mark.parametrize("herd_log2,seed,jb,sb", CASES)
def test_starts_and_steps_record_for_record(K, herd_log2, seed, jb, sb):
    """the starts, then a few hundred steps of the host-compiled kernel arithmetic: the records (dp = 3) and the final state of every
    kangaroo equal the yardstick's; the shared inversion saw no zero"""
    key, base = 0x123456789, 0x100000000
    q = orc.point_of(key)
    mine, want = HostHerd(K, base, q, seed, herd_log2, jb, sb), ref.Herd(base, q, seed, herd_log2, jb, sb)
    try:
        H = 1 << herd_log2
        for i in range(H):
            assert mine.get(i) == (want.x[i], want.y[i], want.d[i]), i
            assert orc.point_of(((key if i & 1 else base) + want.r[i]) % N) == (want.x[i], want.y[i])
        steps = 300 if H <= 2 else 100 if jb < 100 else 20  # (jb = 120: a distance passes 2^128 after some 120 jumps)
        assert sorted(mine.run(steps, 3)) == sorted(want.run(steps, 3))
        for i in range(H):
            assert mine.get(i) == (want.x[i], want.y[i], want.d[i]), i
        assert K.kh_zero_factors(mine.h) == 0 and K.kh_overflow(mine.h) == 0
        # the walk is what it claims: a tame kangaroo stands on (B + d) G, a wild one on (key + d) G
        for i in (0, 1, H - 2, H - 1):
            assert orc.point_of(((key if i & 1 else base) + want.d[i]) % N) == (want.x[i], want.y[i])
    finally:
        mine.close()


def test_distance_overflow_is_reported(K):
    """jb = 120, sb = 124: a distance passes 2^128 within a few hundred jumps - the C step reports the carry where the yardstick raises"""
    q = orc.point_of(5)
    mine, want = HostHerd(K, 1, q, 1, 1, 120, 124), ref.Herd(1, q, 1, 1, 120, 124)
    try:
        done = 0
        with pytest.raises(OverflowError):
            for _ in range(400):
                want.step(32)
                done += 1
        assert 50 < done < 400
        mine.run(done, 32)
        assert K.kh_overflow(mine.h) == 0
        mine.run(1, 32)
        assert K.kh_overflow(mine.h) == 1
    finally:
        mine.close()


def test_distinguished_across_the_limb_boundary(K):
    """herd_is_dp reads limb 0 (bits 0 ... 28) and limb 1 from bit 29 on: for every dp 0 ... 32, on x = 2^b with b on both sides of every dp,
    and on the four constructed points of tests/kangaroo_cases.py, the answer is Python's x & (2^dp - 1) == 0"""
    import kangaroo_cases as kc
    xs = [1 << b for b in range(41)] + [kc.dp_target(name)[2][0] for name in kc.DP_TARGETS]
    xs += [x | 1 << 255 for x in xs[:41]] + [P - 1, 0]
    for x in xs:
        w = words8(x)
        for dp in range(33):
            assert bool(K.kh_is_dp(w.ctypes.data, dp)) == (x & ((1 << dp) - 1) == 0), (hex(x), dp)


def test_a_kangaroo_on_its_own_table_point_takes_the_next_one(K):
    """a kangaroo placed on T_j, and one on -T_j, with j the index its own x picks: the sum would be a doubling / the point at infinity, it takes
    j + 1 mod 32 and lands where the yardstick says; no zero reaches the shared inversion"""
    q, base = orc.point_of(0xABCDEF), 0x1000
    seen = 0
    for seed in range(200):
        s = ref.table(ref.Stream(seed), 20)
        js = [j for j in range(32) if (orc.point_of(s[j])[0] >> 32) & 31 == j]
        if not js:
            continue
        j = js[0]
        tj = orc.point_of(s[j])
        for sign, pt in ((1, tj), (-1, (tj[0], P - tj[1]))):
            mine, want = HostHerd(K, base, q, seed, 3, 20, 30), ref.Herd(base, q, seed, 3, 20, 30)
            try:
                mine.set(5, pt)
                want.x[5], want.y[5] = pt
                d0 = want.d[5]
                assert sorted(mine.run(1, 0)) == sorted(want.run(1, 0))
                assert want.next_rule == 1 and K.kh_zero_factors(mine.h) == 0
                j1 = (j + 1) & 31
                assert want.d[5] == d0 + s[j1] and (want.x[5], want.y[5]) == orc.point_of((sign * s[j] + s[j1]) % N)
                assert mine.get(5) == (want.x[5], want.y[5], want.d[5])
                assert sorted(mine.run(30, 2)) == sorted(want.run(30, 2))
                assert all(mine.get(i) == (want.x[i], want.y[i], want.d[i]) for i in range(8))
            finally:
                mine.close()
        seen += 1
        if seen == 2:
            break
    assert seen == 2


def plan_of(K, a, b, herd_log2=-1, dp=-1):
    A, B, out = arr(a), arr(b), np.zeros(10, np.uint64)
    rc = K.kh_plan(A.ctypes.data, B.ctypes.data, herd_log2, dp, out.ctypes.data)
    if rc:
        return rc, None
    return 0, {"wbits": int(out[0]), "herd_log2": int(out[1]), "dp": int(out[2]), "jb": int(out[3]), "sb": int(out[4]),
               "round_steps": int(out[5]), "base": int_of(out[6:10])}


def test_plan_defaults_limits_and_candidates_on_edge_ranges(K):
    from ecloop_amd import engine
    a0 = 0x1000000000000000000000
    ranges = [(1, 1), (1, 2), (1, 1 << 124), (7, 7), (a0, a0 + (1 << 124) - 1), (1, 1 << 32), (5, 4 + (1 << 48)), (a0, a0 + (1 << 80)),
              (N - 1 - (1 << 40), N - 1), (1 << 20, (1 << 21) - 1)]
    for a, b in ranges:
        for hl, dp in ((None, None), (1, 0), (24, 32), (8, 5), (None, 7), (12, None)):
            rc, p = plan_of(K, a, b, -1 if hl is None else hl, -1 if dp is None else dp)
            want = ref.plan(a, b, hl, dp)
            mine = engine.kangaroo_plan(a, b, hl, dp)
            assert rc == 0 and p == want == {k: mine[k] for k in want}, (a, b, hl, dp)
            assert 1 <= p["herd_log2"] <= 24 and 0 <= p["dp"] <= 32 and 4 <= p["jb"] <= 120 and 1 <= p["sb"] <= 124 and p["base"] == a
            assert p["round_steps"] << p["herd_log2"] <= 1 << 34 or p["round_steps"] == 1
            for mf in (1, 4, 64, 0xFFFFFFFF):
                A, B, lim = arr(a), arr(b), np.zeros(2, np.uint64)
                assert K.kh_give_up(A.ctypes.data, B.ctypes.data, -1 if hl is None else hl, -1 if dp is None else dp, mf, lim.ctypes.data) == 0
                assert int_of(lim) == ref.give_up(want, mf) == engine.kangaroo_give_up(mine, mf)
                assert int_of(lim) == mf * 2 * (1 << -(-want["wbits"] // 2)) + (1 << (want["herd_log2"] + want["dp"]))
    # W = 1, W = 2^124: the edges of what is taken; the defaults as the header's comment gives them
    assert plan_of(K, 9, 9)[1] == {"wbits": 0, "herd_log2": 1, "dp": 0, "jb": 4, "sb": 1, "round_steps": 1, "base": 9}
    p = plan_of(K, a0, a0 + (1 << 124) - 1)[1]
    assert (p["wbits"], p["herd_log2"], p["jb"], p["sb"], p["dp"]) == (124, 22, 82, 124, 32)
    p48 = plan_of(K, 1 << 47, (1 << 48) - 1)[1]
    assert (p48["wbits"], p48["herd_log2"], p48["jb"], p48["sb"], p48["dp"], p48["round_steps"]) == (47, 19, 40, 47, 3, 8)
    p80 = plan_of(K, a0, a0 + (1 << 80) - 1)[1]
    assert (p80["herd_log2"], p80["dp"], p80["jb"]) == (22, 17, 60) and 4 * (1 << 40) >> p80["dp"] <= 1 << 26
    # the refusals: a = 0, a > b, b >= n, W above 2^124, the options
    for a, b, want in ((0, 10, 1), (11, 10, 1), (5, N, 1), (1, N - 1, 2), (a0, a0 + (1 << 124), 2), (1, 1 << 125, 2)):
        assert plan_of(K, a, b)[0] == want, (a, b)
        with pytest.raises(ValueError):
            ref.plan(a, b)
        with pytest.raises(ValueError):
            engine.kangaroo_plan(a, b)
    assert plan_of(K, 1, N - 1)[0] == 2  # b = n - 1 from a = 1 is refused by its width
    assert plan_of(K, N - 1 - (1 << 124) + 1, N - 1)[0] == 0  # ... and taken where the range ends there with 2^124 keys
    for hl, dp in ((0, -1), (25, -1), (-1, 33)):
        assert plan_of(K, 1, 100, hl, dp)[0] == 3
    # the candidates: k = B + d_t - d_w and -(B + d_t) - d_w (mod n), at the limits of the operands
    for base, dt, dw in ((1, 0, 0), (1, 0, 5), (N - 1, (1 << 128) - 1, 0), (N - 1, 0, (1 << 128) - 1), (N - 1, 1, 0), (0x1000, 100, 30),
                         (N - (1 << 127), 1 << 127, 3), (12345, (1 << 128) - 1, (1 << 128) - 1)):
        k1, k2, B, T, W = np.zeros(4, np.uint64), np.zeros(4, np.uint64), arr(base), arr(dt, 2), arr(dw, 2)
        K.kh_candidates(B.ctypes.data, T.ctypes.data, W.ctypes.data, k1.ctypes.data, k2.ctypes.data)
        assert (int_of(k1), int_of(k2)) == ref.candidates(base, dt, dw) == engine.kangaroo_candidates(base, dt, dw), (base, dt, dw)
        assert int_of(k1) == (base + dt - dw) % N and (int_of(k2) + base + dt + dw) % N == 0
    # the pair stands for the key: a tame point (B + d_t) G and a wild one Q + d_w G with equal x, the same point or its negative
    key, base = 0x7777, 0x7000
    assert ref.candidates(base, 0x900, 0x900 - 0x777)[0] == key
    dt = 0x1234
    assert ref.candidates(base, dt, (-(base + dt) - key) % N % (1 << 256))[1] == key


def test_a_whole_search_on_the_host_equals_the_python_driver(K):
    """2^24 keys: the yardstick's driver over the C step (kangaroo_host.cpp) and over its own Python herd give the same key, the same round
    and the same statistics"""
    a, b = 1 << 24, (1 << 25) - 1
    for key, seed in ((a + 0x5A5A5A, 0), (b, 3)):
        q = orc.point_of(key)
        pl = ref.plan(a, b, 5, 3)
        host = HostHerd(K, pl["base"], q, seed, pl["herd_log2"], pl["jb"], pl["sb"])
        try:
            got = ref.search(q, a, b, 5, 3, seed=seed, round_steps=16, run_round=host.run)
            want = ref.search(q, a, b, 5, 3, seed=seed, round_steps=16)
            assert got == want and got[0] == key and K.kh_zero_factors(host.h) == 0, (got, want)
            assert got[1]["rounds"] * 16 * 32 == got[1]["jumps"] < ref.give_up(pl, 64) and got[1]["candidates_checked"] in (1, 2)
        finally:
            host.close()
    # a key outside the range is given up on, at the limit
    q = orc.point_of(a - 12345)
    pl = ref.plan(a, b, 5, 3)
    got, stats = ref.search(q, a, b, 5, 3, seed=1, max_factor=1, round_steps=64)
    assert got is None and ref.give_up(pl, 1) <= stats["jumps"] < ref.give_up(pl, 1) + 64 * 32 and ref.give_up(pl, 1) == 2 * 4096 + 256


def test_header_and_binding_pin_the_flag():
    header = open(os.path.join(ROOT, "include", "ecloop_hip.h")).read()
    assert re.search(r"#define ECL_HERD 2048u\b", header) and "exactly the 45 ecl_hip_* functions" in header and "SIXTEEN limbs" in header
    from ecloop_amd import capi
    assert capi.HERD == 2048 and len(capi.EXPORTS) == 45 and capi.label_of(6) == "dp"
    for kw in ({"herd": True}, {"pub": True, "a33": False, "herd": True, "endo": True}, {"pub": True, "a33": False, "herd": True, "origin": True},
               {"pub": True, "a33": False, "herd": True, "insert": True}, {"pub": True, "herd": True}, {"pub": True, "a33": False, "herd": True, "ord_offs": 33},
               {"a33": False, "eth": True, "herd": True}, {"a33": False, "tr": True, "herd": True}):
        with pytest.raises(ValueError):
            capi.Device(0, **kw)  # refused before the library is asked (no GPU is needed to get here)


def test_the_host_program_runs_clean_under_the_sanitizers(tmp_path):
    """csrc/tools/kangaroo_host.cpp has a main of its own: built as a program with the address and undefined-behaviour sanitizers and run"""
    pr = run_program(host_program(tmp_path, "kangaroo_host.cpp", ["-O0"]))
    assert pr.returncode == 0 and "kangaroo_host: ok" in pr.stdout, (pr.stdout, pr.stderr)


def test_cli_names_the_command_and_refuses_before_a_gpu_is_looked_for(cli, tmp_path):
    out = subprocess.run([cli], capture_output=True, text=True, timeout=60).stdout
    assert re.search(r"^  kangaroo +- ", out, re.M) and all(re.search(r"^  %s <" % f, out, re.M) for f in ("-herd", "-dp", "-seed", "-max")), out
    x, y = orc.point_of(0x9001)
    good = "%02x%064x" % (2 | (y & 1), x)

    def run(*args):
        return subprocess.run([cli, "kangaroo"] + list(args), stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60)
    pr = run("-r", "8000:ffff")
    assert pr.returncode == 1 and "missing -k" in pr.stderr
    pr = run("-k", "%064x" % x, "-r", "8000:ffff")
    assert pr.returncode == 1 and "a bare x names two keys" in pr.stderr
    for rng in ("ffff:8000", "0:ff", "8000", "8000:zz", "1:%x" % ((1 << 124) + 1)):
        pr = run("-k", good, "-r", rng)
        assert pr.returncode == 1 and "invalid search range" in pr.stderr, rng
    pr = run("-k", good, "-r", "8000:ffff", "-t", "2")
    assert pr.returncode == 1 and "one GPU" in pr.stderr
    for flag, bad in (("-dp", "33"), ("-dp", "x"), ("-herd", "0"), ("-herd", "25"), ("-max", "0")):
        pr = run("-k", good, "-r", "8000:ffff", flag, bad)
        assert pr.returncode == 1 and "invalid %s" % flag in pr.stderr, (flag, bad)
    assert run("-k", good, "-r", "8000:ffff", "-q").returncode == 1
