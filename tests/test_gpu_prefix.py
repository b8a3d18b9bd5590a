"""The prefix search (-p, ECL_PREFIX) on the GPU: the prefix kernels' records against the oracle's hashes (tests/eth_ref.py for -a e) and a
table built around them, dense hits through the ring, keys past nkeys, split and strided calls, ecl_hip_diag_bloom against the host
build of prefix.h, the ABI's refusals, key coverage, and the CLI's found lines against the brute-force yardstick tests/prefix_ref.py.
Every GPU-using subprocess runs under its own time limit."""
import ctypes as C
import functools
import hashlib
import random

import numpy as np
import pytest

import eth_ref
import orc
import prefix_ref as R
from fake_device import FakeDevice
from support import cli, host_lib, run_cli

pytestmark = pytest.mark.gpu
START, NKEYS = 0x8000, 4096
TOP = R.TOP
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
WHOLE = np.array([R.words5(0) + R.words5(TOP)], np.uint32)
TYPES = {"c": dict(a33=True), "u": dict(a33=False, a65=True), "cu": dict(a33=True, a65=True), "cu-endo": dict(a33=True, a65=True, endo=True),
         "e": dict(a33=False, eth=True), "e-endo": dict(a33=False, eth=True, endo=True)}


@functools.lru_cache(maxsize=None)
def eth_records(offs=0):
    """(offset, words, endo, 3) of every key x image, by the yardstick: computed once, the plain set is its image 0"""
    from ecloop_amd.engine import calc_priv
    return tuple((off, tuple(eth_ref.eth_words(*orc.point_of(calc_priv(START, 1 << offs, off, e)))), e, 3) for off in range(NKEYS) for e in range(6))


@functools.lru_cache(maxsize=None)
def expected_records(name, start=START, nkeys=NKEYS, offs=0):
    """every record an all-passing filter would give: (offset, h160 words, endo, type)"""
    t = TYPES[name]
    if t.get("eth"):
        assert (start, nkeys) == (START, NKEYS)
        return tuple(r for r in eth_records(offs) if t.get("endo") or r[2] == 0)
    d = FakeDevice(0, a33=t.get("a33", False), a65=t.get("a65", False), endo=t.get("endo", False), ord_offs=offs)
    d.set_bloom(ONES)
    recs, n = d.add_range(start, nkeys, cap=1 << 20)
    assert n == len(recs) == nkeys * (int(t.get("a33", False)) + int(t.get("a65", False))) * (6 if t.get("endo") else 1)
    return tuple((int(r["key_offset"]), tuple(int(w) for w in r["h160"]), int(r["endo"]), int(r["compressed"])) for r in recs)


def keys_of(recs):
    return sorted((int(r["key_offset"]), tuple(int(w) for w in r["h160"]), int(r["endo"]), int(r["compressed"])) for r in recs)


def table_around(values, seed):
    """about 300 sorted disjoint ranges around some of the values: ends exactly on a value, one below and one above it, single values, ranges
    that differ from their neighbours in the last word only, ranges that hold several values, ranges that span many stage-1 buckets"""
    vals = sorted(set(values))
    rng = random.Random(seed)
    far = [i for i in range(2, len(vals) - 2) if vals[i] - vals[i - 1] > 1 << 141 and vals[i + 1] - vals[i] > 1 << 141 and 16 < vals[i] & 0xFFFFFFFF < 0xFFFFFFF0]
    anchors = sorted(rng.sample(far, 280))
    anchors = [i for j, i in enumerate(anchors) if j == 0 or i - anchors[j - 1] > 3]  # (a several-values range reaches two values further)
    pairs, inside, beside = [], 0, 0
    for j, i in enumerate(anchors):
        a, d = vals[i], rng.getrandbits(rng.choice((3, 31, 32, 33, 64, 100, 137, 140))) + 1
        style = j % 7
        if style == 0:
            pairs.append((a - d, a))
            inside += 1
        elif style == 1:
            pairs.append((a, a + d))
            inside += 1
        elif style == 2:
            pairs.append((a - d, a - 1))
            beside += 1
        elif style == 3:
            pairs.append((a + 1, a + d))
            beside += 1
        elif style == 4:
            pairs.append((a, a))
            inside += 1
        elif style == 5:  # three ranges that differ in the last word only; the value sits in the middle one, or between two of them
            if j % 2:
                pairs.extend([(a - 9, a - 1), (a, a), (a + 1, a + 9)])
                inside += 1
            else:
                pairs.extend([(a - 9, a - 1), (a + 1, a + 9)])
                beside += 1
        else:
            pairs.append((a, vals[i + 2]))
            inside += 3
    pairs.sort()
    assert all(p[1] < q[0] for p, q in zip(pairs, pairs[1:])) and all(0 <= lo <= hi <= TOP for lo, hi in pairs)
    assert 180 <= len(pairs) <= 400 and inside > 50 and beside > 50
    return pairs


def members(pairs, records):
    """the records whose value lies inside a range, sorted"""
    inside = R.membership(pairs)
    return sorted(r for r in records if inside(R.value_of(r[1])))


def table_of(pairs):
    return np.array([R.words5(lo) + R.words5(hi) for lo, hi in pairs], np.uint32).reshape(-1, 10)


def open_prefix(name, geometry=None, offs=0):
    from ecloop_amd import Device
    d = Device(0, ord_offs=offs, prefix=True, **{"a33": True, **TYPES[name]})
    if geometry:
        d.set_geometry(*geometry)
    return d


@pytest.mark.parametrize("geometry", [(8, 256), None], ids=["8x256", "auto"])
@pytest.mark.parametrize("name", list(TYPES))
def test_exact_set_parity(name, geometry):
    want_all = expected_records(name)
    pairs = table_around([R.value_of(r[1]) for r in want_all], name)
    want = members(pairs, want_all)
    assert 50 < len(want) < len(want_all) // 10
    d = open_prefix(name, geometry)
    try:
        d.set_prefixes(table_of(pairs))
        before = d.coverage()
        recs, total = d.add_range(START, NKEYS, cap=4096)
        after = d.coverage()
    finally:
        d.close()
    got = keys_of(recs)
    assert total == len(recs) and len(got) == len(set(got))  # no duplicates
    assert got == want  # no false positive, nothing missed, and the values one below / one above a range stay out
    assert tuple(b - a for a, b in zip(before, after)) == (NKEYS, NKEYS, NKEYS)  # requested == covered == counted on the device


@pytest.mark.parametrize("name", ["cu-endo", "e"])
def test_dense_hits_drain_the_ring_at_full_width_and_overflow_keeps_the_rest(name):
    want = sorted(expected_records(name))
    d = open_prefix(name, (8, 256))
    try:
        d.set_prefixes(WHOLE)
        recs, total = d.add_range(START, NKEYS, cap=len(want) + 16)
        assert total == len(recs) == len(want) and keys_of(recs) == want  # every key, every hash, once
        first, total = d.add_range(START, NKEYS, cap=16)  # ECL_E_OVERFLOW: the true total, sixteen records, the rest still on the device
        assert total == len(want) and len(first) == 16
        rest = d.fetch_found(16, total - 16)
        assert len(rest) == total - 16 and keys_of(np.concatenate([first, rest])) == want
    finally:
        d.close()


def test_no_record_past_nkeys():
    want = sorted(r for r in expected_records("cu") if r[0] < 1000)
    for geometry in ((8, 256), None):
        d = open_prefix("cu", geometry)
        try:
            d.set_prefixes(WHOLE)
            recs, total = d.add_range(START, 1000, cap=4096)
            assert total == len(recs) == 2000 and max(int(r["key_offset"]) for r in recs) == 999 and keys_of(recs) == want
            assert d.coverage() == (1000, 1000, 1000)
        finally:
            d.close()


def test_split_calls_and_a_strided_call():
    want_all = expected_records("c")
    pairs = table_around([R.value_of(r[1]) for r in want_all], "split")
    d = open_prefix("c", (8, 256))
    try:
        d.set_prefixes(table_of(pairs))
        one, _ = d.add_range(START, NKEYS)
        a, _ = d.add_range(START, 2048)
        b, _ = d.add_range(START + 2048, 2048)  # contiguous: continues the resident walk
        b = b.copy()
        b["key_offset"] += 2048
        assert keys_of(np.concatenate([a, b])) == keys_of(one) == members(pairs, want_all)
        assert len(a) and len(b)
    finally:
        d.close()
    strided = expected_records("c", 0x123456789ABCDEF, 2048, 12)
    pairs = table_around([R.value_of(r[1]) for r in strided], "strided")
    want = members(pairs, strided)
    assert len(want) > 20
    d = open_prefix("c", offs=12)
    try:
        d.set_prefixes(table_of(pairs))
        recs, total = d.add_range(0x123456789ABCDEF, 2048)
        assert total == len(recs) and keys_of(recs) == want
    finally:
        d.close()


def test_diag_bloom_runs_the_two_stage_prefix_test(tmp_path_factory):
    """the synthetic boundary values of the CPU test (tests/prefix_ref.py: prefix_filter_cases): the device's answers equal the host build's"""
    H = host_lib(tmp_path_factory, "prefix_host.cpp")
    H.px_test_many.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    d = open_prefix("c")
    try:
        for name, (pairs, values) in sorted(R.prefix_filter_cases().items()):
            table = table_of(pairs)
            vals = np.array([R.words5(v) for v in values], np.uint32).reshape(-1, 5)
            s1, host = np.zeros(len(vals), np.uint8), np.zeros(len(vals), np.uint8)
            assert H.px_test_many(table.ctypes.data, len(table), vals.ctypes.data, len(vals), s1.ctypes.data, host.ctypes.data) == 0
            d.set_prefixes(table)
            dev = d.diag_bloom(vals)
            assert (dev == host).all(), name
            assert [int(v) for v in dev] == R.expect(pairs, values)[1], name
    finally:
        d.close()


def test_abi_refusals():
    from ecloop_amd import capi
    lib = capi.load()
    P = capi.PREFIX
    bad = [P, P | capi.ENDO, P | capi.ADDR33 | capi.P2SH, P | capi.P2SH, P | capi.TR, P | capi.PUB, P | capi.PUB | capi.ORIGIN, P | capi.PUB | capi.INSERT,
           P | capi.PUB | capi.HERD, P | capi.ADDR33 | capi.ETH, P | capi.ADDR33 | 8, P | capi.ADDR33 | 8192]
    for flags in bad:
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, flags, 0) == capi.E_ARG, flags
    for flags in (P | capi.ADDR33, P | capi.ADDR65 | capi.ENDO, P | capi.ADDR33 | capi.ADDR65, P | capi.ETH, P | capi.ETH | capi.ENDO):
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, flags, 0) == 0, flags  # (the self-test of the context runs the prefix kernel)
        lib.ecl_hip_close(h)
    h = C.c_void_p()
    assert lib.ecl_hip_open(C.byref(h), 0, P | capi.ADDR33, 0) == 0
    try:
        out, n = np.zeros(16, capi.FOUND_DTYPE), C.c_uint32()
        start = capi.limbs(START)
        add = lambda: lib.ecl_hip_add_range(h, start.ctypes.data, 2048, out.ctypes.data, 16, C.byref(n))
        assert add() == capi.E_NOBLOOM  # no table yet
        t = lambda pairs: table_of(pairs)
        good = t([(5, 9), (20, 30)])
        set_table = lambda tab, nwords: lib.ecl_hip_set_bloom(h, tab.ctypes.data, nwords)  # (tab: C-contiguous, alive in the caller)
        assert set_table(good, 7) == capi.E_ARG and set_table(good, 9) == capi.E_ARG  # no multiple of 5
        many = t([(4 * i, 4 * i + 1) for i in range((1 << 16) + 1)])
        assert set_table(many, 5 * ((1 << 16) + 1)) == capi.E_ARG  # n > 2^16
        assert set_table(t([(9, 5)]), 5) == capi.E_ARG  # lo > hi
        assert set_table(t([(20, 30), (5, 9)]), 10) == capi.E_ARG  # unsorted
        assert set_table(t([(5, 20), (20, 30)]), 10) == capi.E_ARG and set_table(t([(5, 20), (7, 8)]), 10) == capi.E_ARG  # overlapping
        assert add() == capi.E_NOBLOOM  # a refused table leaves the context without one
        assert set_table(many, 5 << 16) == 0 and set_table(good, 10) == 0
        assert add() == 0 and n.value == 0
        hashes = np.zeros((4, 5), np.uint32)
        words = np.zeros(64, np.uint64)
        added = C.c_uint64()
        assert lib.ecl_hip_set_list(h, hashes.ctypes.data, 1) == capi.E_ARG
        assert lib.ecl_hip_bloom_insert(h, hashes.ctypes.data, 4) == capi.E_ARG
        assert lib.ecl_hip_bloom_insert_count(h, hashes.ctypes.data, 4, C.byref(added)) == capi.E_ARG
        assert lib.ecl_hip_get_bloom(h, words.ctypes.data, 64) == capi.E_ARG
        ks = capi.limbs_array([1, 2, 3])
        assert lib.ecl_hip_mul_batch(h, ks.ctypes.data, 3, out.ctypes.data, 16, C.byref(n)) == capi.E_ARG
        text = np.frombuffer(b"abc", np.uint8)
        lines = np.array([3 << 32], np.uint64)
        assert lib.ecl_hip_mul_batch_raw(h, text.ctypes.data, 3, lines.ctypes.data, 1, out.ctypes.data, 16, C.byref(n)) == capi.E_ARG
        assert add() == 0  # ... and the context still works
    finally:
        lib.ecl_hip_close(h)


def test_drop_round_fails_a_prefix_call():
    from ecloop_amd import EclError
    d = open_prefix("c", (8, 256))
    try:
        d.set_prefixes(WHOLE)
        d.add_range(START, NKEYS, cap=NKEYS)
        cov = d.coverage()
        d.diag_drop_round()
        with pytest.raises(EclError) as e:
            d.add_range(START + NKEYS, NKEYS, cap=NKEYS)
        assert e.value.code == -8
        now = d.coverage()
        assert now[0] - cov[0] == NKEYS and now[1] == cov[1] and now[2] - cov[2] < NKEYS
        recs, total = d.add_range(START + NKEYS, NKEYS, cap=NKEYS)  # whole again
        assert total == len(recs) == NKEYS
    finally:
        d.close()


# ---- the CLI

KNOWN = 0xDC2A04
LO, HI = 0xD00000, 0xE00000  # -r d00000:dfffff: 2^20 keys


@pytest.fixture(scope="module")
def hashes33():
    """the oracle's addr33 hashes of the 2^20 keys, as (n, 5) uint32 and as bytes"""
    from ecloop_amd import capi
    h33, _, ok = orc.mul_hash160_many(capi.limbs_array(range(LO, HI)), True, False)
    assert ok.all()
    return h33


def test_cli_add_prints_the_lines_the_yardstick_expects(cli, hashes33, tmp_path):
    known = R.value_of(hashes33[KNOWN - LO])
    assert orc.hex160(hashes33[KNOWN - LO]) == orc.hex160(orc.hash160(*orc.point_of(KNOWN)))
    pattern = R.p2pkh(known)[:6]  # derived from the oracle, not typed in
    raw = np.ascontiguousarray(hashes33.astype(">u4")).tobytes()
    hits = []
    for i in range(HI - LO):  # brute force: every key's address head by base58check, no range arithmetic
        h20 = raw[20 * i:20 * i + 20]
        if (R.p2pkh_head(h20, 6) if h20[0] else R.p2pkh(int.from_bytes(h20, "big"))[:6]) == pattern:
            v = int.from_bytes(h20, "big")
            hits.append(("%040x" % v, "%064x" % (LO + i), R.p2pkh(v)))
    want = ["addr33: %s <- %s %s" % h for h in hits]
    assert "addr33: %040x <- %064x %s" % (known, KNOWN, R.p2pkh(known)) in want
    outfile = tmp_path / "found.txt"
    r = run_cli(cli, ["add", "-p", pattern, "-r", "%x:%x" % (LO, HI - 1), "-o", str(outfile)], timeout=300)
    assert r.found == sorted(want), (r.stdout, r.status)
    assert "filter: prefix (1 pattern, " in r.stdout and "edge: " in r.status
    assert sorted(outfile.read_text().splitlines()) == sorted("addr33\t%s\t%s\t%s" % h for h in hits)  # a fourth tab-separated field
    # the bc1q form (-a c): the same keys' P2WPKH addresses, six characters after the q
    bech = R.p2wpkh(known)[:10]
    top = known >> 130
    want = ["addr33: %040x <- %064x %s" % (R.value_of(h), LO + i, R.p2wpkh(R.value_of(h)))
            for i, h in enumerate(hashes33) if int(h[0]) >> 2 == top and R.p2wpkh(R.value_of(h)).startswith(bech)]
    r = run_cli(cli, ["add", "-p", bech, "-a", "c", "-r", "%x:%x" % (LO, HI - 1)], timeout=300)
    assert r.found == sorted(want) and len(want) >= 1, (r.stdout, r.status)
    # a file of patterns, upper-case bech32 first: the address is written in the form of the first pattern it matches
    f = tmp_path / "patterns.txt"
    f.write_text("%s\n%s\n" % (bech.upper(), pattern))
    r = run_cli(cli, ["add", "-p", str(f), "-r", "%x:%x" % (LO, HI - 1)], timeout=300)
    assert "addr33: %040x <- %064x %s" % (known, KNOWN, R.p2wpkh(known).upper()) in r.found and "prefix (2 patterns, " in r.stdout


def test_cli_add_eth_and_rnd(cli, hashes33):
    lo, n = 0xDC2000, 4096
    addr = {k: R.value_of(eth_ref.eth_words(*orc.point_of(k))) for k in range(lo, lo + n)}
    pattern = R.eth(addr[KNOWN])[:8]  # six digits
    want = sorted("eth: %040x <- %064x %s" % (v, k, R.eth(v)) for k, v in addr.items() if R.eth(v).startswith(pattern))
    assert len(want) >= 1
    r = run_cli(cli, ["add", "-p", pattern.upper().replace("0X", "0x"), "-a", "e", "-r", "%x:%x" % (lo, lo + n - 1)], timeout=300)
    assert r.found == want and "~ eth: 1 | filter: prefix" in r.stdout, (r.stdout, r.status)
    # rnd: one window with a fixed seed; the 2^20 values of the window's offsets cover d00000 ... dfffff, so the known key is in it
    known = R.value_of(hashes33[KNOWN - LO])
    pattern = R.p2pkh(known)[:6]
    r = run_cli(cli, ["rnd", "-p", pattern, "-seed", "prefix", "-r", "%x:%x" % (LO, HI - 1), "-d", "0:20"], env={"ECLOOP_HIP_RND_WINDOWS": "1"}, timeout=300)
    assert "addr33: %040x <- %064x %s" % (known, KNOWN, R.p2pkh(known)) in r.found, (r.stdout, r.status)
    for line in r.found:  # every line is a key of the walk with its own hash and an address that starts with the pattern
        _, h, _, k, a = line.split()
        assert orc.hex160(orc.hash160(*orc.point_of(int(k, 16)))) == h and a == R.p2pkh(int(h, 16)) and a.startswith(pattern)
