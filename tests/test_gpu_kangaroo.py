"""`kangaroo` on the GPU: the flag through the C ABI, the herd's records bit for bit against tests/kangaroo_ref.py (pure Python over the
oracle's points), continuation and re-building, the zero-difference rule, overflow and fetch, the coverage check, and the search end to
end through engine.kangaroo_search (statistics equal to the yardstick's driver) and the CLI.  Every GPU-using subprocess runs under its
own time limit."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import kangaroo_ref as ref
import orc
from support import run_cli

pytestmark = pytest.mark.gpu
P, N = orc.P, orc.N
KEY, BASE = 0x123456789, 0x100000000


def herd_device(dp):
    from ecloop_amd import Device
    return Device(0, a33=False, pub=True, herd=True, ord_offs=dp)


def rec_set(recs):
    return sorted((int(r["key_offset"]), tuple(int(v) for v in r["h160"]), int(r["endo"]), int(r["compressed"])) for r in recs)


def compressed_of(key):
    x, y = orc.point_of(key)
    return "%02x%064x" % (2 | (y & 1), x)


@functools.lru_cache(maxsize=None)
def yardstick(hl, seed, jb, sb, dp, steps, key=KEY, base=BASE):
    herd = ref.Herd(base, orc.point_of(key), seed, hl, jb, sb)
    return tuple(sorted(herd.run(steps, dp))), herd.next_rule


def test_flags_through_the_c_abi():
    from ecloop_amd import capi
    lib = capi.load()
    for dp in (0, 32):
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, capi.PUB | capi.HERD, dp) == 0
        lib.ecl_hip_close(h)
    bad = [(capi.HERD, 0), (capi.HERD | capi.ENDO, 0), (capi.PUB | capi.HERD | capi.ENDO, 0), (capi.PUB | capi.HERD | capi.ORIGIN, 0),
           (capi.PUB | capi.HERD | capi.INSERT, 0), (capi.PUB | capi.HERD, 33), (capi.PUB | capi.HERD, 255)]
    bad += [(capi.PUB | capi.HERD | other, 0) for other in (1, 2, 16, 64, 128)] + [(capi.HERD | other, 0) for other in (1, 2, 16, 64, 128)]
    for flags, dp in bad:
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, flags, dp) == capi.E_ARG and not h, (flags, dp)
    q = orc.point_of(KEY)
    good = (BASE, q, 3, 1, 10, 12)
    d = herd_device(3)
    try:
        for call in (lambda: d.mul_batch([1, 2, 3]), lambda: d.mul_batch_raw([b"abc"])):
            with pytest.raises(capi.EclError) as e:
                call()
            assert e.value.code == capi.E_ARG
        refused = [((BASE, off_curve, 3, 1, 10, 12), 64) for off_curve in ((q[0], (q[1] + 1) % P), (q[0], P), (P, q[1]), ((q[0] + 1) % P, q[1]))]
        refused += [((BASE, q, 3, hl, jb, sb), 1 << 25) for hl, jb, sb in ((0, 10, 12), (25, 10, 12), (1, 3, 12), (1, 121, 12), (1, 10, 0), (1, 10, 125))]
        refused += [(good, 63), (good, 1), ((BASE, q, 3, 7, 10, 12), 128 * 5 + 64)]  # nkeys no multiple of the herd
        for k, (blk, nkeys) in enumerate(refused):
            with pytest.raises(capi.EclError) as e:
                d.add_range(None, nkeys, herd=blk)
            assert e.value.code == capi.E_ARG, (blk, nkeys)
            # ... and the context is whole after each refusal (seeds in turn, so that every call builds its herd); no filter was ever set
            recs, n = d.add_range(None, 2 * 40, cap=256, herd=(BASE, q, 3 + k % 2, 1, 10, 12))
            assert n == len(recs) and rec_set(recs) == list(yardstick(1, 3 + k % 2, 10, 12, 3, 40)[0]), k
        with pytest.raises(ValueError):
            d.add_range(0x8000, 16)
    finally:
        d.close()


@pytest.mark.parametrize("hl,seed,jb,sb,steps", [(1, 3, 10, 12, 300), (7, 9, 20, 30, 100), (12, 5, 30, 40, 64)], ids=["H2", "H128", "H4096"])
def test_records_bit_for_bit(hl, seed, jb, sb, steps):
    """one partly filled lane, a tail wave, many lanes: the sorted records of a call equal the yardstick's exactly, and the coverage totals
    grow by exactly the jumps asked for"""
    want, _ = yardstick(hl, seed, jb, sb, 3, steps)
    d = herd_device(3)
    try:
        before = d.coverage()
        recs, n = d.add_range(None, steps << hl, cap=len(want) + 64, herd=(BASE, orc.point_of(KEY), seed, hl, jb, sb))
        grown = tuple(b - a for a, b in zip(before, d.coverage()))
    finally:
        d.close()
    assert n == len(recs) == len(want) and rec_set(recs) == list(want)
    assert all(int(r["compressed"]) == 6 for r in recs) and grown == (steps << hl,) * 3


def test_continuation_and_rebuilding():
    """two calls of s steps equal one call of 2 s, with one set-up; another seed or another target builds the herd anew (a set-up each) and the
    result is the yardstick's of that block"""
    q, hl, s = orc.point_of(KEY), 7, 50
    blk = (BASE, q, 9, hl, 20, 30)
    d = herd_device(3)
    try:
        d.reset_timing()
        r1, _ = d.add_range(None, s << hl, cap=4096, herd=blk)
        r2, _ = d.add_range(None, s << hl, cap=4096, herd=blk)
        assert d.setup_timing()[1] == 1
        assert rec_set(np.concatenate([r1, r2])) == list(yardstick(hl, 9, 20, 30, 3, 2 * s)[0])
        assert rec_set(r1) == list(yardstick(hl, 9, 20, 30, 3, s)[0])
        r3, _ = d.add_range(None, s << hl, cap=4096, herd=(BASE, q, 10, hl, 20, 30))  # another seed
        assert d.setup_timing()[1] == 2 and rec_set(r3) == list(yardstick(hl, 10, 20, 30, 3, s)[0])
        other = KEY + 77
        r4, _ = d.add_range(None, s << hl, cap=4096, herd=(BASE, orc.point_of(other), 10, hl, 20, 30))  # another target
        assert d.setup_timing()[1] == 3 and rec_set(r4) == list(yardstick(hl, 10, 20, 30, 3, s, key=other)[0])
        r5, _ = d.add_range(None, s << hl, cap=4096, herd=blk)  # the first block again: from its start
        assert d.setup_timing()[1] == 4 and rec_set(r5) == rec_set(r1)
    finally:
        d.close()


def test_zero_difference_on_the_device():
    """Q = (s_j - r_1) G puts wild kangaroo 1 on T_j with j the index its own x picks: it takes j + 1, the shared inversion of its lane sees no
    zero, and the records of 64 steps - its own and the rest of the herd's - are the yardstick's"""
    hl, jb, sb = 7, 20, 30
    for seed in range(500):
        s, r = ref.distances_and_offsets(seed, hl, jb, sb)
        js = [j for j in range(32) if (orc.point_of(s[j])[0] >> 32) & 31 == j and (s[j] - r[1]) % N]
        if js:
            break
    key = (s[js[0]] - r[1]) % N
    q = orc.point_of(key)
    herd = ref.Herd(BASE, q, seed, hl, jb, sb)
    assert (herd.x[1], herd.y[1]) == orc.point_of(s[js[0]])
    want = sorted(herd.run(64, 0))  # dp = 0: every jump is a record
    assert herd.next_rule >= 1 and len(want) == 64 << hl
    d = herd_device(0)
    try:
        recs, n = d.add_range(None, 64 << hl, cap=len(want) + 64, herd=(BASE, q, seed, hl, jb, sb))
    finally:
        d.close()
    assert n == len(want) and rec_set(recs) == want
    # kangaroo 1's first jump: T_j + T_j+1, the distance r_1 + s_j+1
    nxt = s[(js[0] + 1) & 31]
    first = ref.record(1, r[1] + nxt, orc.point_of((s[js[0]] + nxt) % N)[0])
    assert first in want and first in rec_set(recs)


def test_overflow_and_fetch():
    """dp = 0: every jump is a record.  A small cap gives the total with E_OVERFLOW status, fetch_found the rest; the union is the yardstick's"""
    hl, steps = 7, 16
    want, _ = yardstick(hl, 9, 20, 30, 0, steps)
    assert len(want) == steps << hl
    d = herd_device(0)
    try:
        recs, n = d.add_range(None, steps << hl, cap=100, herd=(BASE, orc.point_of(KEY), 9, hl, 20, 30))
        assert n == steps << hl and len(recs) == 100
        rest = d.fetch_found(100, n - 100)
    finally:
        d.close()
    assert len(rest) == n - 100 and rec_set(np.concatenate([recs, rest])) == list(want)


def test_coverage_check_on_the_herd():
    from ecloop_amd import capi
    blk = (BASE, orc.point_of(KEY), 9, 7, 20, 30)
    d = herd_device(3)
    try:
        d.diag_drop_round()
        with pytest.raises(capi.EclError) as e:
            d.add_range(None, 50 << 7, cap=4096, herd=blk)
        assert e.value.code == capi.E_COVERAGE
        requested, covered, device = d.coverage()
        assert (requested, covered, device) == (50 << 7, 0, 49 << 7)
        recs, n = d.add_range(None, 50 << 7, cap=4096, herd=blk)  # the call after that is whole and correct: the herd from its start
        assert rec_set(recs) == list(yardstick(7, 9, 20, 30, 3, 50)[0]) and d.coverage() == (100 << 7, 50 << 7, 99 << 7)
    finally:
        d.close()


A32, B32 = 0x7000000000, 0x7000000000 + (1 << 32) - 1


def inside_key(odd):
    k = A32 + 0x3C0FFEE1
    while (orc.point_of(k)[1] & 1) != odd:
        k += 1
    return k


@functools.lru_cache(maxsize=None)
def yardstick_search(key):
    return ref.search(orc.point_of(key), A32, B32, 8, 5, seed=1, round_steps=64)


@pytest.mark.parametrize("which", ["a", "b", "inside-even-y", "inside-odd-y", "uncompressed"])
def test_end_to_end_exact(which):
    """W = 2^32, H = 2^8, dp = 5, rounds of 64 steps: engine.kangaroo_search returns the key with the statistics of the yardstick's driver"""
    from ecloop_amd import engine
    key = {"a": A32, "b": B32, "inside-even-y": inside_key(0), "inside-odd-y": inside_key(1), "uncompressed": inside_key(1)}[which]
    pub = "04%064x%064x" % orc.point_of(key) if which == "uncompressed" else compressed_of(key)
    want_key, want = yardstick_search(key)
    got_key, got = engine.kangaroo_search(pub, A32, B32, herd_log2=8, dp_bits=5, seed=1, round_steps=64)
    print(which, got)
    assert want_key == key == got_key and got == want


def jumps_of(stderr):
    return int(re.sub(r"\D", "", re.findall(r"jumps: ([^~]+) ~", stderr)[-1]))


def test_end_to_end_defaults_through_the_cli(tmp_path):
    """W = 2^48 with the default herd (2^20) and dp (3): the CLI prints the `pub:` line and writes the -o line for a key in the range, within
    64 * 2 sqrt(W) = 2^31 jumps (seed 7: see the figure the run prints; the limit is the condition); a target outside the range ends with
    `not found within ... jumps` and status 0 at -max 4"""
    from ecloop_amd import engine
    from ecloop_amd.build import build_host_cli
    a, b = 0x1000000000000, 0x1000000000000 + (1 << 48) - 1
    key = a + 0x5EED5EED5EED
    plan = engine.kangaroo_plan(a, b)
    assert (plan["herd_log2"], plan["dp"]) == (20, 3)
    out = tmp_path / "found.txt"
    pr = run_cli(build_host_cli(), ["kangaroo", "-k", compressed_of(key), "-r", "%x:%x" % (a, b), "-seed", "7", "-o", str(out)], hard_limit=120)
    line = "pub: %s <- %064x" % (compressed_of(key), key)
    assert line in pr.stdout.split("\n") and out.read_text() == "pub\t%s\t%064x\n" % (compressed_of(key), key)
    jumps = jumps_of(pr.stderr)
    print("jumps to the key:", jumps)
    assert 0 < jumps < 64 * 2 * (1 << 24)
    outside = b + (1 << 60)
    pr = run_cli(build_host_cli(), ["kangaroo", "-k", compressed_of(outside), "-r", "%x:%x" % (a, b), "-seed", "7", "-max", "4"], hard_limit=120)
    limit = engine.kangaroo_give_up(plan, 4)
    m = re.search(r"^%s not found within (\d+) jumps$" % compressed_of(outside), pr.stderr, re.M)
    assert m and limit <= int(m.group(1)) < limit + (plan["round_steps"] << plan["herd_log2"]) and "pub:" not in pr.stdout
