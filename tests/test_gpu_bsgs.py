"""`bsgs` on the GPU: the two flags through the C ABI, the origin walk key by key against tests/pub_ref.py (pure Python over the oracle's
points), geometries and continuation, the insert walk's filter bit for bit against the host's, the search end to end through
engine.bsgs_search and the CLI with keys planted at every edge of the windows, a thin filter whose false positives are the yardstick's,
and the coverage check on both new contexts.  Every GPU-using subprocess runs under its own time limit."""
import ctypes as C

import numpy as np
import pytest

import orc
import pub_ref
from support import rec_set, run_cli

pytestmark = pytest.mark.gpu
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
P, N = orc.P, orc.N
T_KEY = 0xdc2a04  # the origin of most tests: O = T_KEY G


def origin_device(words=ONES, offs=0):
    from ecloop_amd import Device
    d = Device(0, a33=False, pub=True, origin=True, ord_offs=offs)
    d.set_bloom(words)
    return d


def insert_device(nwords, offs=1):
    from ecloop_amd import Device
    d = Device(0, a33=False, pub=True, insert=True, ord_offs=offs)
    d.set_bloom(np.zeros(nwords, np.uint64))
    return d


def walk_x(k0, step, count):
    """x of (k0 + i step) G, i < count: two of the oracle's points, then affine additions in Python integers"""
    x, y = orc.point_of(k0 % N)
    sx, sy = orc.point_of(step % N)
    out = []
    for _ in range(count):
        out.append(x)
        lam = (sy - y) * pow(sx - x, -1, P) % P
        x3 = (lam * lam - x - sx) % P
        x, y = x3, (lam * (x - x3) - y) % P
    return out


def host_filter(nwords, xs):
    from ecloop_amd import engine
    words = np.zeros(nwords, np.uint64)
    engine.blf_add_host(words, np.array([pub_ref.words5(x) for x in xs], np.uint32))
    return words


def test_flags_through_the_c_abi():
    from ecloop_amd import Device, capi
    lib = capi.load()
    for flags in (capi.PUB | capi.ORIGIN, capi.PUB | capi.INSERT):  # (each runs its self-test)
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, flags, 0) == 0, flags
        lib.ecl_hip_close(h)
    for new in (capi.ORIGIN, capi.INSERT):
        bad = [capi.PUB | new | capi.ENDO, capi.PUB | capi.ORIGIN | capi.INSERT, new, new | capi.ENDO]
        bad += [capi.PUB | new | other for other in (1, 2, 16, 64, 128)] + [new | other for other in (1, 2, 16, 64, 128)]
        for flags in bad:
            h = C.c_void_p()
            assert lib.ecl_hip_open(C.byref(h), 0, flags, 0) == capi.E_ARG and not h, flags
    for d in (origin_device(), insert_device(1024)):
        try:
            with pytest.raises(capi.EclError) as e:
                d.mul_batch([1, 2, 3])
            assert e.value.code == capi.E_ARG
            with pytest.raises(capi.EclError) as e:
                d.mul_batch_raw([b"abc"])
            assert e.value.code == capi.E_ARG
        finally:
            d.close()
    d = origin_device()
    try:
        x, y = orc.point_of(T_KEY)
        for off_curve in ((x, (y + 1) % P), (x, P), (P, y), ((x + 1) % P, y)):
            with pytest.raises(capi.EclError) as e:
                d.add_range(0x8000, 4096, origin=off_curve)
            assert e.value.code == capi.E_ARG, off_curve
        recs, n = d.add_range(0x8000, 16, cap=64, origin=(x, y))  # ... and the context is whole afterwards
        assert n == 16
        with pytest.raises(ValueError):
            d.add_range(0x8000, 16)
    finally:
        d.close()


@pytest.mark.parametrize("start,nkeys,offs", [(0x3F000, 5000, 0), (0x51234, 4096, 12)], ids=["contiguous", "stride4096"])
def test_origin_walk_every_key_once(start, nkeys, offs):
    """all-ones filter, O = t G: exactly one record per key, h160 = the yardstick's x of start + off 2^offs + t; the coverage totals grow by
    the keys asked"""
    d = origin_device(offs=offs)
    try:
        before = d.coverage()
        recs, n = d.add_range(start, nkeys, cap=nkeys + 16, origin=orc.point_of(T_KEY))
        grown = tuple(b - a for a, b in zip(before, d.coverage()))
    finally:
        d.close()
    assert n == len(recs) == nkeys and sorted(int(r["key_offset"]) for r in recs) == list(range(nkeys))
    assert all(int(r["compressed"]) == 5 and int(r["endo"]) == 0 for r in recs)
    assert grown == (nkeys, nkeys, nkeys)
    for r in recs:
        assert tuple(int(v) for v in r["h160"]) == pub_ref.h160_of(start + (int(r["key_offset"]) << offs) + T_KEY), int(r["key_offset"])


def test_origin_geometries_change_no_record():
    """half group 2 with 256 lanes and a ragged count, the geometry the origin is chosen for, a larger half group, the automatic one: the same
    records, each the yardstick's.  The origin t G makes E + O = 4 D under the geometry 8 x 256 (E = C_0 - D, D = 2 B G): lane 3 of
    k_init_centres_table meets its own cached multiple and takes the complete formulas"""
    B, T = 8, 256
    k0 = 0x7_0000_0000
    t = (4 * 2 * B - (k0 + B - 2 * B)) % N  # E's scalar is k0 + B - 2B
    nkeys = 2 * B * T * 2 + 77
    sets = []
    for geo in ((8, 256), (2, 256), (64, 512), None):
        d = origin_device()
        try:
            if geo:
                d.set_geometry(*geo)
            recs, n = d.add_range(k0, nkeys, cap=nkeys + 16, origin=orc.point_of(t))
            assert n == len(recs) == nkeys, (geo, n)
            sets.append(rec_set(recs))
        finally:
            d.close()
    assert all(s == sets[0] for s in sets[1:])
    want = [tuple(pub_ref.words5(x)) for x in walk_x(k0 + t, 1, nkeys)]
    assert [s[3] for s in sets[0]] == want and [s[0] for s in sets[0]] == list(range(nkeys))
    assert want[0] == pub_ref.h160_of(k0 + t) and want[-1] == pub_ref.h160_of(k0 + t + nkeys - 1)


def test_origin_continuation_and_a_change_of_origin():
    """two contiguous calls with one origin continue the resident walk (one set-up) and equal the single call; a third contiguous call with
    another origin re-positions (a second set-up) and is right as well"""
    sweep, k0 = 2 * 8 * 256, 0x9_0000_0000
    o1, o2 = orc.point_of(T_KEY), orc.point_of(N - 77)
    d = origin_device()
    try:
        d.set_geometry(8, 256)
        whole, n = d.add_range(k0, 2 * sweep, cap=2 * sweep, origin=o1)
        assert n == 2 * sweep
    finally:
        d.close()
    d = origin_device()
    try:
        d.set_geometry(8, 256)
        a, na = d.add_range(k0, sweep, cap=sweep, origin=o1)
        s1 = d.setup_timing()[1]
        b, nb = d.add_range(k0 + sweep, sweep, cap=sweep, origin=o1)
        s2 = d.setup_timing()[1]
        c, nc = d.add_range(k0 + 2 * sweep, sweep, cap=sweep, origin=o2)
        s3 = d.setup_timing()[1]
    finally:
        d.close()
    assert (na, nb, nc) == (sweep,) * 3 and (s1, s2, s3) == (1, 1, 2)
    assert sorted(rec_set(a) + rec_set(b, sweep)) == rec_set(whole)
    assert [x[3] for x in rec_set(whole)] == [tuple(pub_ref.words5(x)) for x in walk_x(k0 + T_KEY, 1, 2 * sweep)]
    assert [x[3] for x in rec_set(c)] == [tuple(pub_ref.words5(x)) for x in walk_x(k0 + 2 * sweep - 77, 1, sweep)]


@pytest.mark.parametrize("nkeys,geo", [(1000, (8, 256)), (1 << 16, None)], ids=["1000-of-4096-walked", "65536-auto"])
def test_insert_builds_the_host_filter_bit_for_bit(nkeys, geo):
    """a zeroed filter of 4099 words, start 1, ord_offs 1: afterwards it equals the filter the host builds from x((2j - 1) G), j <= nkeys -
    no bit of key nkeys + 1 onward, which the walk computes as well (the geometry 8 x 256 walks 4096); nothing is reported, the keys are counted"""
    d = insert_device(4099)
    try:
        if geo:
            d.set_geometry(*geo)
        before = d.coverage()
        recs, n = d.add_range(1, nkeys, cap=16)
        grown = tuple(b - a for a, b in zip(before, d.coverage()))
        got = d.get_bloom(4099)
    finally:
        d.close()
    assert n == 0 and len(recs) == 0 and grown == (nkeys, nkeys, nkeys)
    xs = walk_x(1, 2, nkeys + 8)
    assert xs[1] == orc.point_of(3)[0] and xs[nkeys - 1] == orc.point_of(2 * nkeys - 1)[0]
    want = host_filter(4099, xs[:nkeys])
    assert (got == want).all()
    if nkeys == 1000:  # (at 2^16 keys the 4099 words are 99 % ones: eight keys more need not show there)
        assert not (host_filter(4099, xs[:nkeys + 8]) == want).all()  # the next keys, which the walk computed too, would have shown


def compressed_of(k):
    return pub_ref.compressed(k)


def run_bsgs(args):
    """-> the `pub: ` lines in the order they were printed, stderr"""
    from ecloop_amd.build import build_host_cli
    r = run_cli(build_host_cli(), ["bsgs"] + args, hard_limit=120)
    return [l for l in r.stdout.splitlines() if l.startswith("pub: ")], r.stderr


def test_end_to_end_keys_at_every_edge(tmp_path):
    """beta = 10 over 2^24 keys: keys at a and b, the last key of window 5 and the first of window 6, a + 7 s + h - 1, both parities of y, and
    a range whose length is no multiple of s with its last key - each found by engine.bsgs_search and printed by the CLI as
    pub: <Q> <- <key>; a Q whose key is b + 1 is reported not found after all N steps"""
    from ecloop_amd import engine
    beta, a = 10, 0x1_0000_0000_0000
    h, s = 1 << beta, 2 << beta
    b = a + (1 << 24) - 1
    steps = (1 << 24) // s
    keys = [a, b, a + 6 * s - 1, a + 6 * s, a + 7 * s + h - 1, a + 1234567]
    k = a + 99 * s + 5
    while {orc.point_of(x)[1] & 1 for x in keys} != {0, 1}:  # one key of each parity of y
        keys.append(k)
        k += 1
    for key in keys:
        got, stats = engine.bsgs_search(compressed_of(key), a, b, baby_log2=beta)
        assert got == key, hex(key)
        assert stats["baby_keys"] == h and stats["giant_steps"] == steps and stats["windows_rescanned"] == stats["false_positives"] + 1, stats
    got, stats = engine.bsgs_search(compressed_of(b + 1), a, b, baby_log2=beta)
    assert got is None and stats["giant_steps"] == steps and stats["windows_rescanned"] == stats["false_positives"], stats
    # uncompressed keys too
    x, y = orc.point_of(keys[2])
    assert engine.bsgs_search("04%064x%064x" % (x, y), a, b, baby_log2=beta)[0] == keys[2]
    # a length that is no multiple of s: its last key, and the key behind it - which lies in the last window and is not in the range
    b2 = b - 777
    got, stats = engine.bsgs_search(compressed_of(b2), a, b2, baby_log2=beta)
    assert got == b2 and stats["giant_steps"] == steps
    got, stats = engine.bsgs_search(compressed_of(b2 + 1), a, b2, baby_log2=beta)
    assert got is None and stats["giant_steps"] == steps
    # the CLI: all keys of the range from one file, then the ragged range
    listed = tmp_path / "targets.txt"
    listed.write_text("".join(compressed_of(key) + "\n" for key in keys + [b + 1]))
    out = tmp_path / "found.txt"
    lines, err = run_bsgs(["-k", str(listed), "-r", "%x:%x" % (a, b), "-b", str(beta), "-o", str(out)])
    assert lines == [pub_ref.found_line(key) for key in keys], (lines, err)
    assert err.count("not found") == 1 and compressed_of(b + 1) + " not found" in err
    assert out.read_text().splitlines() == ["pub\t%s\t%064x" % (compressed_of(key), key) for key in keys]
    lines, err = run_bsgs(["-k", compressed_of(b2), "-r", "%x:%x" % (a, b2), "-b", str(beta)])
    assert lines == [pub_ref.found_line(b2)] and "not found" not in err
    lines, err = run_bsgs(["-k", compressed_of(b2 + 1), "-r", "%x:%x" % (a, b2), "-b", str(beta)])
    assert lines == [] and compressed_of(b2 + 1) + " not found" in err and "%d / %d" % (steps, steps) in err.replace(",", "")
    # the default beta and filter
    lines, err = run_bsgs(["-k", compressed_of(keys[4]), "-r", "%x:%x" % (a, b)])
    assert lines == [pub_ref.found_line(keys[4])]


def test_false_positives_of_a_thin_filter_are_the_yardsticks():
    """beta = 10, 256 filter words (16 bits per entry: a giant step passes by chance with p = 1.2e-3), 2^14 giant steps.  A target outside the
    range walks every step: the false positives counted equal the yardstick's - the Python bloom over the x of every W_i - and nothing is
    found.  Then, with the same filter, a target in the last window: found, after the yardstick's false positives before it.
    (The two targets are s keys apart, so one walk of x values serves both: W_i of the first is W_(i-1) of the second.)"""
    from ecloop_amd import engine
    beta, a, nsteps = 10, 0x2_0000_0000_0000, 1 << 14
    h, s = 1 << beta, 2 << beta
    b = a + nsteps * s - 1
    inside = b - 100          # in the last window
    outside = inside + s      # not in the range
    plan = engine.bsgs_plan(a, b, beta)
    assert plan["steps"] == nsteps
    words = host_filter(256, walk_x(1, 2, h))
    # X[j + 1] = x((giant_start + 2 s j - 2 inside) G), j = -1 ... nsteps - 1
    X = walk_x(plan["giant_start"] - 2 * s - 2 * inside, 2 * s, nsteps + 1)
    assert X[1] == pub_ref.x_of(plan["giant_start"] - 2 * inside) and X[nsteps] == pub_ref.x_of(plan["giant_start"] + 2 * s * (nsteps - 1) - 2 * inside)
    idx = engine.blf_indices(np.array([pub_ref.words5(x) for x in X], np.uint32))
    bit = (words[((idx >> np.uint64(6)) % np.uint64(256)).astype(np.int64)] >> (idx & np.uint64(63))) & np.uint64(1)
    passes = bit.all(axis=1)
    fp_outside = [i for i in range(nsteps) if passes[i]]           # W_i = X[i]
    fp_inside = [i for i in range(nsteps - 1) if passes[i + 1]]    # W_i = X[i + 1]; step nsteps - 1 is the true hit
    baby = set(walk_x(1, 2, h))
    assert passes[nsteps] and X[nsteps] in baby and not any(X[i] in baby for i in fp_outside) and not any(X[i + 1] in baby for i in fp_inside)
    print("yardstick false positives:", len(fp_outside), len(fp_inside))
    assert len(fp_outside) >= 3 and len(fp_inside) >= 3
    got, stats = engine.bsgs_search(pub_ref.compressed(outside), a, b, baby_log2=beta, filter_words=256)
    assert got is None and stats["giant_steps"] == nsteps, stats
    assert stats["false_positives"] == stats["windows_rescanned"] == len(fp_outside), (stats, len(fp_outside))
    got, stats = engine.bsgs_search(pub_ref.compressed(inside), a, b, baby_log2=beta, filter_words=256)
    assert got == inside and stats["false_positives"] == len(fp_inside) and stats["windows_rescanned"] == len(fp_inside) + 1, (stats, len(fp_inside))


def test_a_dropped_round_fails_the_call_on_both_contexts():
    """ecl_hip_diag_drop_round on an origin context and on an insert context: ECL_E_COVERAGE, and the next call is whole"""
    from ecloop_amd import capi
    o = orc.point_of(T_KEY)
    d = origin_device()
    try:
        d.set_geometry(8, 256)
        d.diag_drop_round()
        with pytest.raises(capi.EclError) as e:
            d.add_range(0x3F000, 5000, cap=8192, origin=o)
        assert e.value.code == capi.E_COVERAGE
        recs, n = d.add_range(0x3F000, 5000, cap=8192, origin=o)
        assert n == 5000 and [x[3] for x in rec_set(recs)] == [tuple(pub_ref.words5(x)) for x in walk_x(0x3F000 + T_KEY, 1, 5000)]
        assert d.coverage()[:2] == (10000, 5000)
    finally:
        d.close()
    d = insert_device(4099)
    try:
        d.set_geometry(8, 256)
        d.diag_drop_round()
        with pytest.raises(capi.EclError) as e:
            d.add_range(1, 1000, cap=16)
        assert e.value.code == capi.E_COVERAGE
        recs, n = d.add_range(1, 1000, cap=16)
        assert n == 0 and (d.get_bloom(4099) == host_filter(4099, walk_x(1, 2, 1000))).all()
        assert d.coverage()[:2] == (2000, 1000)
    finally:
        d.close()
