"""`bsgs` (baby-step giant-step for a known public key; ECL_ORIGIN, ECL_INSERT) without a GPU: the plan arithmetic the CLI runs
(host/bsgs_plan.h), the origin addition of the set-up kernel (csrc/ec.h: ec_add_origin) and the bit positions of the insert walk
(csrc/pub_emit.h: pub_insert_idx), all compiled for the host (csrc/tools/bsgs_host.cpp), against a brute-force restatement in Python over
the oracle's points; the pins of the C ABI header and the binding; the CLI's refusals; the new kernels' registers from the kept assembly."""
import ctypes as C
import functools
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import orc
import pub_ref
from ecloop_amd.capi import limbs
from support import ROOT, cli, host_lib, host_program, int_of, kept_assembly, run_program, words8

sys.path.insert(0, os.path.join(ROOT, "tools"))
P, N = orc.P, orc.N


def ptr(v):
    """the limbs of v as a pointer argument that keeps its array alive for the call"""
    return limbs(v).ctypes.data_as(C.c_void_p)


def words16(pt):
    return words8(pt[0]) + words8(pt[1])


@functools.lru_cache(maxsize=None)
def x_of(k):
    return pub_ref.x_of(k)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    lib = host_lib(tmp_path_factory, "bsgs_host.cpp")
    lib.bh_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
    lib.bh_default_beta.argtypes = [C.c_void_p, C.c_void_p]
    lib.bh_default_beta.restype = C.c_uint
    lib.bh_giant_call.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
    lib.bh_giant_call.restype = C.c_uint64
    lib.bh_window.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
    lib.bh_window.restype = C.c_uint64
    lib.bh_lift_x.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.bh_on_curve.argtypes = [C.c_void_p, C.c_void_p]
    lib.bh_origin.argtypes = [C.c_void_p] * 4
    lib.bh_origin.restype = None
    lib.bh_origin_add_many.argtypes = [C.c_void_p] * 4 + [C.c_uint32]
    lib.bh_origin_add_many.restype = None
    lib.bh_insert_idx_many.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    lib.bh_insert_idx_many.restype = None
    return lib


def plan_of(H, a, b, beta):
    """-> (rc, plan as a dict) from the C header"""
    A, B, out = limbs(a), limbs(b), np.zeros(18, np.uint64)
    rc = H.bh_plan(A.ctypes.data, B.ctypes.data, beta, out.ctypes.data)
    if rc:
        return rc, None
    return 0, {"h": int(out[0]), "s": int(out[1]), "baby_offs": int(out[2]), "baby_keys": int(out[3]), "giant_offs": int(out[4]),
               "filter_words": int(out[5]), "steps": int_of(out[6:10]), "baby_start": int_of(out[10:14]), "giant_start": int_of(out[14:18])}


def window_of(H, a, b, beta, i):
    first = np.zeros(4, np.uint64)
    n = H.bh_window(ptr(a), ptr(b), beta, ptr(i), first.ctypes.data)
    return int_of(first), int(n)


SWEEP = 1024  # the smallest sweep a walk can have: 256 lanes of one group of half group 2 - a call walks up to the next multiple of it


def test_plan_coverage_every_key_of_a_small_grid(H):
    """every (a, b, beta) of the grid, every key of [a, b]: the giant step W_i = (giant_start + i 2^giant_offs) G - 2Q, as the yardstick's x of
    the scalar (pub_ref.x_of over the oracle's points), meets the baby set {x((2j - 1) G), j <= h} in exactly the window that holds the key,
    the windows tile [a, b], and no step of the walked extent - padded to a sweep - is the point at infinity or claims the key"""
    from ecloop_amd import engine
    checked = 0
    for beta in (0, 1, 2, 3):
        h, s = 1 << beta, 2 << beta
        baby = {x_of(2 * j - 1) for j in range(1, h + 1)}
        odd = set(range(1, 2 * h, 2))
        for a in (1, 2, 7, 0x8000):
            for length in range(1, 41):
                b = a + length - 1
                rc, p = plan_of(H, a, b, beta)
                assert rc == 0, (a, b, beta)
                mine = engine.bsgs_plan(a, b, beta)
                assert {k: p[k] for k in p} == {k: mine[k] for k in p}, (a, b, beta)
                n = p["steps"]
                assert (p["h"], p["s"], n) == (h, s, -(-length // s)) and p["giant_start"] == 2 * a + s - 1 and p["giant_offs"] == beta + 2
                assert (p["baby_start"], p["baby_offs"], p["baby_keys"]) == (1, 1, h)
                # the windows tile [a, b]
                at = a
                for i in range(n):
                    first, nk = window_of(H, a, b, beta, i)
                    assert first == at == a + i * s and nk == min(s, b - first + 1), (a, b, beta, i)
                    at += nk
                assert at == b + 1
                padded = -(-n // SWEEP) * SWEEP
                for key in range(a, b + 1):
                    home = (key - a) // s
                    for i in range(n):  # on points: the yardstick's x of the step
                        w = (p["giant_start"] + (i << p["giant_offs"]) - 2 * key) % N
                        x = x_of(w)
                        assert x is not None, (a, b, beta, key, i)
                        assert (x in baby) == (i == home), (a, b, beta, key, i)
                        checked += 1
                    for i in range(n, padded):  # the padding: by the scalar (a step meets the baby set iff its scalar is +-(2j - 1))
                        w = (p["giant_start"] + (i << p["giant_offs"]) - 2 * key) % N
                        assert w != 0 and w not in odd and N - w not in odd, (a, b, beta, key, i)
    assert checked == 4 * sum(length * -(-length // (2 << beta)) for beta in (0, 1, 2, 3) for length in range(1, 41)) == 87984
    # the scalar rule used for the padding, on points
    assert all((x_of(w) in {x_of(1), x_of(3)}) == (w in (1, 3, N - 1, N - 3)) for w in list(range(1, 12)) + [N - 1, N - 2, N - 3, N - 4])


def test_plan_refusals_chunks_and_default_beta(H):
    from ecloop_amd import engine
    for beta in (0, 3, 10, 30):
        s = 2 << beta
        edge = (N - 1) // 2 - s  # the first b with 2 (b + s) + 1 >= n
        assert 2 * (edge + s) + 1 >= N > 2 * (edge - 1 + s) + 1
        for b, want in ((edge - 1, 0), (edge, 2), (edge + 5, 2), (N - 1, 2)):
            assert plan_of(H, 5, b, beta)[0] == want, (beta, hex(b))
            if want:
                with pytest.raises(ValueError):
                    engine.bsgs_plan(5, b, beta)
    for a, b in ((0, 10), (11, 10), (5, N), (5, N + 3)):
        assert plan_of(H, a, b, 3)[0] == 1, (a, b)
    # a wide range in calls of at most 2^32 steps
    a, beta = 0x1000000000000000000000, 30
    b = a + (1 << 80) + 12345
    rc, p = plan_of(H, a, b, beta)
    n = p["steps"]
    assert rc == 0 and n == -(-(b - a + 1) // p["s"]) and n > 1 << 48
    for done in (0, 1 << 32, 5 << 32, n - (n % (1 << 32)), n - 1):
        start = np.zeros(4, np.uint64)
        got = H.bh_giant_call(ptr(a), ptr(b), beta, ptr(done), start.ctypes.data)
        assert got == min(1 << 32, n - done) and int_of(start) == p["giant_start"] + done * 2 * p["s"], done
    assert H.bh_giant_call(ptr(a), ptr(b), beta, ptr(n), np.zeros(4, np.uint64).ctypes.data) == 0
    assert window_of(H, a, b, beta, n - 1) == (a + (n - 1) * p["s"], b - (a + (n - 1) * p["s"]) + 1)
    # the default: ceil((bits(b - a + 1) - 1) / 2) clamped to 10 ... 30; the filter: one word per baby step, 1024 at least
    for length, want in ((1, 10), (1 << 19, 10), (1 << 20, 10), ((1 << 21) - 1, 10), (1 << 21, 11), (1 << 24, 12), (1 << 59, 30), (1 << 80, 30), (1 << 200, 30)):
        bits = length.bit_length()
        assert want == min(30, max(10, -(-(bits - 1) // 2)))
        assert H.bh_default_beta(ptr(7), ptr(7 + length - 1)) == want == engine.bsgs_default_beta(7, 7 + length - 1), length
    assert plan_of(H, 1, 100, 3)[1]["filter_words"] == 1024 and plan_of(H, 1, 1 << 40, 20)[1]["filter_words"] == 1 << 20


def test_lift_and_origin_of_the_plan_header(H):
    """y of a compressed key and O = -2Q, against the oracle's points; x on no point and x >= p are refused"""
    from ecloop_amd import engine
    rnd = random.Random(9)
    for k in [1, 2, 3, 0xdc2a04, N - 1, N - 2] + [rnd.randrange(1, N) for _ in range(40)]:
        x, y = orc.point_of(k)
        got = np.zeros(4, np.uint64)
        for odd in (0, 1):
            assert H.bh_lift_x(ptr(x), odd, got.ctypes.data) == 1
            assert int_of(got) == (y if (y & 1) == odd else P - y)
        assert H.bh_on_curve(ptr(x), ptr(y)) == 1 and H.bh_on_curve(ptr(x), ptr((y + 1) % P)) == 0
        ox, oy = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
        H.bh_origin(ptr(x), ptr(y), ox.ctypes.data, oy.ctypes.data)
        assert (int_of(ox), int_of(oy)) == orc.point_of((N - 2 * k) % N) == engine.bsgs_origin((x, y)), k
        assert engine.bsgs_point("%02x%064x" % (2 | (y & 1), x)) == (x, y) == engine.bsgs_point("04%064x%064x" % (x, y))
    x = 5
    while pow((x ** 3 + 7) % P, (P - 1) // 2, P) == 1:
        x += 1
    got = np.zeros(4, np.uint64)
    assert H.bh_lift_x(ptr(x), 0, got.ctypes.data) == 0 and H.bh_lift_x(ptr(P), 0, got.ctypes.data) == 0
    assert H.bh_on_curve(ptr(P + 1), ptr(2)) == 0
    for bad in ("%064x" % orc.point_of(5)[0], "02%064x" % x, "04%064x%064x" % (orc.point_of(5)[0], 1), "05" + "%064x" % orc.point_of(5)[0]):
        with pytest.raises(ValueError):
            engine.bsgs_point(bad)


def test_origin_addition_of_the_device_function(H):
    """ec_add_origin, the function k_origin_add runs: O = t G added to E = e G is (e + t) G; E = O is the doubling; E with the x of O and
    the other y is reported (0) and nothing is stored in its place"""
    rnd = random.Random(512)
    es = [1, 2, 0xdc2a04, N - 1] + [rnd.randrange(1, N) for _ in range(60)]
    ts = [7, N - 3, 0x123456789abcdef] + [rnd.randrange(1, N) for _ in range(61)]
    cases = [(e, t) for e, t in zip(es, ts) if (e + t) % N and (e - t) % N]
    cases += [(e, e) for e in es[:8]]          # the doubling
    cases += [(e, N - e) for e in es[:8]]      # E = -O
    E = np.array([words16(orc.point_of(e)) for e, _ in cases], np.uint32)
    O = np.array([words16(orc.point_of(t)) for _, t in cases], np.uint32)
    out = np.full((len(cases), 16), 0xA5A5A5A5, np.uint32)
    fin = np.full(len(cases), 7, np.uint32)
    H.bh_origin_add_many(E.ctypes.data, O.ctypes.data, out.ctypes.data, fin.ctypes.data, len(cases))
    seen = {"add": 0, "dbl": 0, "inf": 0}
    for i, (e, t) in enumerate(cases):
        if (e + t) % N == 0:
            assert fin[i] == 0 and (out[i] == 0xA5A5A5A5).all(), (e, t)
            seen["inf"] += 1
            continue
        assert fin[i] == 1 and [int(v) for v in out[i]] == words16(orc.point_of((e + t) % N)), (e, t)
        seen["dbl" if e == t else "add"] += 1
    assert seen["add"] > 50 and seen["dbl"] == 8 and seen["inf"] == 8


def test_pub_insert_sets_the_bits_the_probe_reads(H):
    """pub_insert_idx: the 20 positions equal engine.blf_indices of the yardstick's five words, at every magnitude a walked x arrives in"""
    from ecloop_amd import engine
    rnd = random.Random(1024)
    xs = [P - 1, P - 2, 1, 0, 0xFF, (1 << 224) + 5, 1 << 255] + [x_of(k) for k in (1, 3, 5, 2047)] + [rnd.randrange(P) for _ in range(500)]
    X = np.array([words8(x) for x in xs], np.uint32)
    want = engine.blf_indices(np.array([pub_ref.words5(x) for x in xs], np.uint32))
    for mag in (1, 2, 4):
        idx = np.zeros((len(xs), 20), np.uint64)
        H.bh_insert_idx_many(X.ctypes.data, mag, idx.ctypes.data, len(xs))
        assert (idx == want).all(), mag


def test_header_and_binding_pin_the_two_flags():
    header = open(os.path.join(ROOT, "include", "ecloop_hip.h")).read()
    assert re.search(r"#define ECL_ORIGIN 512u\b", header) and re.search(r"#define ECL_INSERT 1024u\b", header)
    assert "exactly the 45 ecl_hip_* functions" in header and "TWELVE limbs" in header
    from ecloop_amd import capi
    assert capi.ORIGIN == 512 and capi.INSERT == 1024 and len(capi.EXPORTS) == 45
    for kw in ({"origin": True}, {"insert": True}, {"pub": True, "a33": False, "origin": True, "insert": True},
               {"pub": True, "a33": False, "origin": True, "endo": True}, {"pub": True, "a33": False, "insert": True, "endo": True}):
        with pytest.raises(ValueError):
            capi.Device(0, **kw)  # refused before the library is asked (no GPU is needed to get here)


def test_the_host_program_runs_clean_under_the_sanitizers(tmp_path):
    """csrc/tools/bsgs_host.cpp has a main of its own: built as a program with the address and undefined-behaviour sanitizers and run"""
    pr = run_program(host_program(tmp_path, "bsgs_host.cpp", ["-O0"]))
    assert pr.returncode == 0 and "bsgs_host: ok" in pr.stdout, (pr.stdout, pr.stderr)


def test_cli_names_the_command_and_refuses_before_a_gpu_is_looked_for(cli, tmp_path):
    out = subprocess.run([cli], capture_output=True, text=True, timeout=60).stdout
    assert re.search(r"^  bsgs +- ", out, re.M) and all(re.search(r"^  %s <" % f, out, re.M) for f in ("-k", "-b", "-m")), out
    x, y = orc.point_of(0x9001)
    good = "%02x%064x" % (2 | (y & 1), x)

    def run(*args):
        return subprocess.run([cli, "bsgs"] + list(args), stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60)
    pr = run("-k", "%064x" % x, "-r", "8000:ffff")
    assert pr.returncode == 1 and "a bare x names two keys" in pr.stderr
    listed = tmp_path / "keys.txt"
    listed.write_text(good + "\n04%064x%064x\n" % (x, (y + 1) % P))
    for key, msg in (("05" + good[2:], "invalid public key"), ("04%064x%064x" % (x, (y + 1) % P), "invalid public key"), (str(listed), "invalid public key")):
        pr = run("-k", key, "-r", "8000:ffff")
        assert pr.returncode == 1 and msg in pr.stderr, pr.stderr
    pr = run("-k", good, "-r", "8000:ffff", "-t", "2")
    assert pr.returncode == 1 and "one GPU" in pr.stderr
    pr = run("-k", good, "-r", "8000:%x" % ((N - 1) // 2))
    assert pr.returncode == 1 and "2 (b + s) + 1 >= n" in pr.stderr
    for rng in ("ffff:8000", "0:ff", "8000", "8000:zz"):
        pr = run("-k", good, "-r", rng)
        assert pr.returncode == 1 and "invalid search range" in pr.stderr, rng
    assert run("-r", "8000:ffff").returncode == 1 and run("-k", good, "-r", "8000:ffff", "-q").returncode == 1


def test_the_new_kernels_registers_and_loops():
    """static, from the assembly the build keeps (tools/isa_mix.py --bsgs): the insert walk fits 128 VGPRs (four waves per SIMD, as
    k_add_pub), has no scratch instruction below its launch loop, sets its 20 bits in the `which` loop, and its loop nest was seen; the
    origin kernel does not spill.  Figures of this build: 128 VGPRs, 14 spilled (launch loop), per key 1 536 static VALU against 813."""
    import isa_mix
    now = isa_mix.analyse_bsgs(kept_assembly())
    ins, org = now["bsgs insert"], now["bsgs origin"]
    print(ins["registers"], ins["per_key_valu"], ins["pub_per_key_valu"], org["registers"])
    assert ins["registers"]["vgpr_count"] <= 128 and ins["scratch_below_top"] == 0
    assert any(l["depth"] >= 3 for l in ins["loops"]) and ins["which_loop_vmem"] == 20
    assert ins["per_key_valu"] > ins["pub_per_key_valu"] > 0
    assert org["registers"]["vgpr_spill_count"] == 0
