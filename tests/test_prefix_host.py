"""The prefix search (-p, ECL_PREFIX) without a GPU: the planner (host/prefix_plan.h through csrc/tools/prefix_host.cpp, and its mirror
engine.prefix_ranges) against the brute-force yardstick tests/prefix_ref.py; the device filter prefix.h compiled for the host against
Python; the CLI's refusals, help text and 2^-16 bound; the binding."""
import bisect
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import prefix_ref as R
from support import ROOT, cli, host_lib

TOP = R.TOP
H1 = R.value_of([0x751E76E8, 0x199196D4, 0x54941C45, 0xD1B3A323, 0xF1433BD6])  # hash160 of the compressed key of 1
A1 = "1BgGZ9tcN4rm9KBzDn7KprQz87SZ26SAMH"
W1 = "bc1qw508d6qejxtdg4y5r3zarvary0c5xw7kv8f3t4"

# (pattern, a33, a65, eth): several leading 1s, two digit counts, 30 characters, bc1q with 1 and 32 characters, 0x with 1 and 40 digits
B58_PATTERNS = ["1Lo", "1z", "12", "11a", "1Q", "111", "1111", "1QLbz7", "1Love", "1QLbz7JHiBTsp", "11111a", A1[:30], A1, "1111111111111111111114oL"]
PATTERNS = [(p, True, False, False) for p in B58_PATTERNS] + [("1Lov", False, True, False), ("1zz", True, True, False)] + \
    [(p, True, False, False) for p in ("bc1qq", "bc1qw508", "BC1QW508D", W1[:36])] + \
    [(p, False, False, True) for p in ("0x0", "0xdead", "0xDeAdBeEf", "0x%040x" % H1)]


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    lib = host_lib(tmp_path_factory, "prefix_host.cpp")
    lib.px_test_many.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.px_table_ok.argtypes = [C.c_void_p, C.c_uint64]
    lib.px_bitmap_popcount.argtypes = [C.c_void_p, C.c_uint32]
    lib.px_bitmap_popcount.restype = C.c_uint64
    lib.px_pattern_ranges.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_char_p]
    lib.px_plan.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p]
    lib.px_address.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]
    lib.px_match.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_char_p]
    lib.px_sha256.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p]
    return lib


def c_pattern_ranges(H, p, a33, a65, eth):
    """-> list of (lo, hi), or (code, message)"""
    out = np.zeros((36, 10), np.uint32)
    why = C.create_string_buffer(320)
    n = H.px_pattern_ranges(p.encode(), a33, a65, eth, out.ctypes.data, why)
    if n < 0:
        return n, why.value.decode()
    return [(R.value_of(r[:5]), R.value_of(r[5:])) for r in out[:n]]


def c_plan(H, patterns, a33, a65, eth):
    cap = 1024
    table = np.zeros((cap, 10), np.uint32)
    at, serve = np.zeros(cap + 1, np.uint32), np.zeros(cap * 8, np.uint32)
    why = C.create_string_buffer(320)
    n = H.px_plan("\n".join(patterns).encode(), a33, a65, eth, table.ctypes.data, cap, at.ctypes.data, serve.ctypes.data, why)
    if n < 0:
        return n, why.value.decode()
    return table[:n].copy(), [[int(v) for v in serve[at[i]:at[i + 1]]] for i in range(n)]


def test_the_yardstick_knows_the_public_vectors(H):
    assert R.p2pkh(H1) == A1 and R.p2wpkh(H1) == W1 and R.p2pkh(0) == "1111111111111111111114oLvT2"
    assert R.eth(0x7E5F4552091A69125D5DFCB7B8C2659029395BDF) == "0x7e5f4552091a69125d5dfcb7b8c2659029395bdf"
    assert R.b58_decode(A1)[1:21] == H1.to_bytes(20, "big")
    rng = random.Random(3)
    for v in [H1, TOP, 1 << 152] + [rng.getrandbits(160) | 1 << 152 for _ in range(2000)]:
        n = rng.randrange(1, 12)
        assert R.p2pkh_head(v.to_bytes(20, "big"), n) == R.p2pkh(v)[:n]
    # ... and so does the host code the CLI prints a hit with (its own SHA-256, base58 and bech32)
    import hashlib
    rng = random.Random(1)
    for msg in [b"", b"abc", bytes(55), bytes(56), bytes(64), bytes(rng.randrange(256) for _ in range(200))]:
        out = C.create_string_buffer(32)
        H.px_sha256(msg, len(msg), out)
        assert out.raw == hashlib.sha256(msg).digest(), len(msg)
    for v in [0, 1, TOP, H1, 0xFF << 152, 1 << 151] + [rng.getrandbits(160) >> rng.choice((0, 0, 8, 17, 64)) for _ in range(300)]:
        w = np.array(R.words5(v), np.uint32)
        buf = C.create_string_buffer(48)
        for form, upper, want in ((1, 0, R.p2pkh(v)), (2, 0, R.p2wpkh(v)), (2, 1, R.p2wpkh(v).upper()), (3, 0, R.eth(v))):
            H.px_address(w.ctypes.data, form, upper, buf)
            assert buf.value.decode() == want, (hex(v), form)


def matching_values(pattern, rng, count):
    """values whose address starts with a base58 pattern, found without the planner's arithmetic: the pattern plus random digits is decoded,
    the hash inside it re-encoded (its own checksum), and kept if the text still starts with the pattern"""
    out = []
    for total in range(max(len(pattern), 26), 36):
        for _ in range(count):
            s = pattern + "".join(rng.choice(R.B58) for _ in range(total - len(pattern)))
            raw = R.b58_decode(s)
            if len(raw) != 25 or raw[0] != 0:
                continue
            v = int.from_bytes(raw[1:21], "big")
            if R.matches(pattern, v):
                out.append(v)
    return out


@pytest.mark.parametrize("pattern,a33,a65,eth", PATTERNS, ids=[p[0] for p in PATTERNS])
def test_planner_against_the_yardstick(H, pattern, a33, a65, eth):
    from ecloop_amd import engine
    ranges = c_pattern_ranges(H, pattern, a33, a65, eth)
    assert isinstance(ranges, list), ranges
    assert ranges == engine.prefix_pattern_ranges(pattern, a33, a65, eth)  # the mirror, range by range
    merged = sorted(set(ranges))
    rng = random.Random(pattern)
    inside = lambda v: any(lo <= v <= hi for lo, hi in merged)
    # (1) no value whose address starts with the pattern lies outside: random values, and values built to match
    cands = [rng.getrandbits(160) for _ in range(20000)]
    if pattern[0] == "1":
        cands += [rng.getrandbits(160 - 8 * z) for z in (1, 2, 3, 4) for _ in range(3000)] + matching_values(pattern, rng, 40)
        if len(pattern) > 3 or pattern.startswith("11"):
            assert any(R.matches(pattern, v) for v in cands)  # (the construction does find some)
    hits = 0
    for v in cands:
        if R.matches(pattern, v):
            hits += 1
            assert inside(v), hex(v)
    if pattern in ("1Lo", "1z", "12", "1Q", "0x0", "bc1qq"):
        assert hits > 0
    # (2) every interior value of a range matches; only its first and last value may not; (3) the values next to a range do not match
    for lo, hi in merged:
        assert 0 <= lo <= hi <= TOP
        probe = {lo + 1, hi - 1, (lo + hi) // 2} | {rng.randrange(lo, hi + 1) for _ in range(50)}
        for v in probe:
            if lo < v < hi:
                assert R.matches(pattern, v), (hex(lo), hex(v), hex(hi))
        for v in (lo - 1, hi + 1):
            if 0 <= v <= TOP and not inside(v):
                assert not R.matches(pattern, v), hex(v)


def test_patterns_that_need_two_digit_counts_and_leading_ones(H):
    assert len(c_pattern_ranges(H, "1QLbz7", True, False, False)) == 2  # 33 and 34 characters
    assert len(c_pattern_ranges(H, "1Lo", True, False, False)) <= 2 and len(c_pattern_ranges(H, "1z", True, False, False)) <= 2
    assert c_pattern_ranges(H, "111", True, False, False) == [(0, (1 << 144) - 1)]  # at least two zero bytes
    (lo, hi), = c_pattern_ranges(H, "11a", True, False, False)  # exactly one zero byte
    assert lo >> 152 == 0 and hi >> 152 == 0 and lo >> 144 > 0
    assert c_pattern_ranges(H, "1" * 21, True, False, False) == [(0, 0)]


REFUSALS = [
    ("1l", True, False, False, -1, "base58 alphabet"), ("1O0", True, False, False, -1, "base58 alphabet"), ("1I", True, False, False, -1, "base58 alphabet"),
    ("bc1qb", True, False, False, -1, "bech32 alphabet"), ("bc1qQ", True, False, False, -1, "mixed case"), ("0xg", False, False, True, -1, "hex digit"),
    ("1" * 23, True, False, False, -2, "no address can start"), ("1" + "z" * 34, True, False, False, -2, "no address can start"),
    ("1zzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzz", True, False, False, -2, "no address can start"),  # 34 characters, above the largest address
    ("bc1q" + "q" * 33, True, False, False, -2, "no address can start"), ("0x" + "0" * 41, False, False, True, -2, "no address can start"),
    ("hello", True, False, False, -2, "no address can start"), ("", True, False, False, -2, "no address can start"),
    ("1Love", False, False, True, -3, "needs -a c, u or cu"), ("bc1qw5", True, True, False, -3, "needs -a c"), ("bc1qw5", False, True, False, -3, "needs -a c"),
    ("0xdead", True, False, False, -3, "needs -a e"),
    ("3J98", True, False, False, -4, "not supported yet"), ("bc1pmfr3", True, False, False, -4, "not supported yet"), ("deadbeef", False, False, True, -4, "not supported yet"),
]


@pytest.mark.parametrize("pattern,a33,a65,eth,code,reason", REFUSALS, ids=["%s/%d" % (r[0][:12], i) for i, r in enumerate(REFUSALS)])
def test_refusals_name_the_pattern_and_the_reason(H, pattern, a33, a65, eth, code, reason):
    from ecloop_amd import engine
    got = c_pattern_ranges(H, pattern, a33, a65, eth)
    assert isinstance(got, tuple) and got[0] == code and reason in got[1] and "'%s'" % pattern in got[1], got
    with pytest.raises(engine.PrefixError) as e:
        engine.prefix_ranges([pattern], a33, a65, eth)
    assert str(e.value) == got[1]


def test_the_bound_is_computed_not_guessed(H):
    from ecloop_amd import engine
    # exactly 2^-16 passes, anything above it does not: 0x with 4 and 3 digits, bc1q with 4 and 3 characters (2^-20, 2^-15), '111' (2^-16)
    for p, a33, eth, ok in (("0xdead", False, True, True), ("0xdea", False, True, False), ("bc1qw508", True, False, True), ("bc1qw50", True, False, False),
                            ("111", True, False, True), ("11", True, False, False), ("1Q", True, False, False), ("1z", True, False, False),
                            ("1Lo", True, False, False), ("1Love", True, False, True)):
        got = c_plan(H, [p], a33, False, eth)
        assert (isinstance(got[0], np.ndarray)) == ok, (p, got)
        if not ok:
            assert got[0] == -5 and "2^-16" in got[1] and "lengthen" in got[1] and "'%s'" % p in got[1]
            with pytest.raises(engine.PrefixError) as e:
                engine.prefix_ranges([p], a33, False, eth)
            assert str(e.value) == got[1]
    # the sum over several patterns counts: two halves of 2^-16 pass, a third pattern beside them does not
    assert isinstance(c_plan(H, ["0xdead0", "0xdead1", "0xdead2", "0xdead3", "0xdead4", "0xdead5", "0xdead6", "0xdead7"], False, False, True)[0], np.ndarray)
    assert c_plan(H, ["0xdead", "0xbeef0"], False, False, True)[0] == -5
    assert isinstance(c_plan(H, ["0xdead", "0xdead0"], False, False, True)[0], np.ndarray)  # overlap is not counted twice


SETS = [(["1Love", "1QLbz7", "1Love1"], True, False, False), (["0xdead0", "0xdead1", "0xdeae0", "0xDEAD15"], False, False, True),
        (["bc1qw508d", "1BgGZ9", "bc1qw508e", "BC1QW508D6"], True, False, False), (["1QLbz7", "1QLbz8", "1QLbz6"], True, True, False),
        ([A1], True, False, False), (["0x%040x" % H1, "0x%040x" % (H1 + 1), "0x%040x" % (H1 + 3)], False, False, True)]


@pytest.mark.parametrize("patterns,a33,a65,eth", SETS, ids=[s[0][0][:10] for s in SETS])
def test_c_planner_and_python_mirror_give_identical_tables(H, patterns, a33, a65, eth):
    from ecloop_amd import engine
    table, serves = c_plan(H, patterns, a33, a65, eth)
    ptable, pserves = engine.prefix_ranges(patterns, a33, a65, eth)
    assert table.dtype == ptable.dtype == np.uint32 and table.shape == ptable.shape and (table == ptable).all()
    assert serves == pserves
    assert table.flags.c_contiguous and H.px_table_ok(table.ctypes.data, len(table)) == 1
    pairs = [(R.value_of(r[:5]), R.value_of(r[5:])) for r in table]
    for (l0, h0), (l1, h1) in zip(pairs, pairs[1:]):
        assert h0 + 1 < l1  # merged: neither overlapping nor adjacent
    # each range serves the patterns whose own ranges lie in it, and no other
    for (lo, hi), s in zip(pairs, serves):
        want = sorted(i for i, p in enumerate(patterns) if any(lo <= a and b <= hi for a, b in engine.prefix_pattern_ranges(p, a33, a65, eth)))
        assert s == want
    # a hit's text is written in the form of the first pattern it matches, in list order
    rng = random.Random(7)
    for lo, hi in pairs:
        for v in {lo, hi, (lo + hi) // 2, rng.randrange(lo, hi + 1)}:
            for typ, label in ((3, "eth"),) if eth else ((1, "addr33"), (0, "addr65")):
                buf = C.create_string_buffer(48)
                w = np.array(R.words5(v), np.uint32)  # (a name keeps the array alive over the call)
                got = H.px_match("\n".join(patterns).encode(), a33, a65, eth, w.ctypes.data, typ, buf)
                want = next((i for i, p in enumerate(patterns) if not (p[:2].lower() == "bc" and typ != 1) and R.matches(p, v)), -1)
                assert got == want, (hex(v), typ)
                text = engine.prefix_match(patterns, R.words5(v), label)
                assert (text is None) == (want < 0)
                if want >= 0:
                    assert buf.value.decode() == text == R.address(patterns[want], v)


def test_adjacent_and_overlapping_ranges_merge(H):
    table, serves = c_plan(H, ["0xdead0", "0xdead1", "0xdead15"], False, False, True)
    assert len(table) == 1 and serves == [[0, 1, 2]]
    assert R.value_of(table[0][:5]) == 0xDEAD0 << 140 and R.value_of(table[0][5:]) == (0xDEAD2 << 140) - 1


# ---- the device filter, compiled for the host

def run_filter(H, pairs, values):
    table = np.array([R.words5(lo) + R.words5(hi) for lo, hi in pairs], np.uint32).reshape(-1, 10)
    vals = np.array([R.words5(v) for v in values], np.uint32).reshape(-1, 5)
    s1, hit = np.zeros(len(vals), np.uint8), np.zeros(len(vals), np.uint8)
    assert H.px_test_many(table.ctypes.data, len(table), vals.ctypes.data, len(vals), s1.ctypes.data, hit.ctypes.data) == 0
    return s1, hit


CASES = R.prefix_filter_cases()
expect = R.expect


@pytest.mark.parametrize("name", sorted(CASES))
def test_prefix_filter_for_the_host_against_python(H, name):
    pairs, values = CASES[name]
    s1, hit = run_filter(H, pairs, values)
    want_s1, want = expect(pairs, values)
    assert [int(v) for v in hit] == want
    assert [int(v) for v in s1] == want_s1
    assert all(a >= b for a, b in zip(want_s1, want))  # stage 1 never rejects a hit
    assert sum(want) > 0 and (name == "whole" or sum(want) < len(want))  # the case asks both kinds of question
    if name == "straddle":
        table = np.array([R.words5(lo) + R.words5(hi) for lo, hi in pairs], np.uint32)
        assert H.px_bitmap_popcount(table.ctypes.data, len(pairs)) == 9  # buckets e-1, e | e, e+1 | e+4 ... e+9 of the three ranges: e is shared


def test_table_check(H):
    def ok(pairs):
        table = np.array([R.words5(lo) + R.words5(hi) for lo, hi in pairs], np.uint32)  # (a name keeps the array alive over the call)
        return H.px_table_ok(table.ctypes.data, len(pairs))
    assert ok([(5, 9)]) == 1 and ok([(5, 5), (6, 6)]) == 1 and ok([(0, TOP)]) == 1
    assert ok([(9, 5)]) == 0  # lo > hi
    assert ok([(10, 20), (5, 8)]) == 0  # unsorted
    assert ok([(10, 20), (20, 30)]) == 0 and ok([(10, 20), (15, 16)]) == 0 and ok([(10, 20), (10, 20)]) == 0  # overlapping
    assert ok([(1 << 128, 1 << 129), ((1 << 128) - 1, 1 << 130)]) == 0  # the most significant word decides
    empty = np.zeros(10, np.uint32)
    assert H.px_table_ok(empty.ctypes.data, 0) == 0
    many = [(i * 4, i * 4 + 1) for i in range((1 << 16) + 1)]
    assert ok(many[:1 << 16]) == 1 and ok(many) == 0


# ---- the CLI (no GPU is reached: everything here is decided before a device is opened)

def refused(cli, args):
    pr = subprocess.run([cli] + args, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=120)
    assert pr.returncode == 1, (args, pr.stdout, pr.stderr)
    return pr.stderr


def test_cli_refusals_and_help(cli, tmp_path):
    assert "-p and -f exclude each other" in refused(cli, ["add", "-p", "1Love", "-f", "x.blf", "-r", "1000:2000"])
    assert "-p is not supported with mul" in refused(cli, ["mul", "-p", "1Love"])
    for a in ("s", "t", "x", "cs"):
        assert "-p is not supported with -a %s" % a in refused(cli, ["add", "-p", "1Love", "-a", a, "-r", "1000:2000"])
    assert "pattern '1l0ve': a character outside the base58 alphabet" in refused(cli, ["add", "-p", "1l0ve", "-r", "1000:2000"])
    assert "pattern '3J98t1': P2SH patterns (3...) are not supported yet" in refused(cli, ["add", "-p", "3J98t1", "-r", "1000:2000"])
    assert "pattern 'bc1pmfr3': Taproot patterns (bc1p...) are not supported yet" in refused(cli, ["rnd", "-p", "bc1pmfr3"])
    assert "bare hex patterns are not supported yet" in refused(cli, ["add", "-p", "deadbeef", "-a", "e", "-r", "1000:2000"])
    assert "a 0x pattern needs -a e" in refused(cli, ["add", "-p", "0xdeadbeef", "-r", "1000:2000"])
    assert "a bc1q pattern needs -a c" in refused(cli, ["add", "-p", "bc1qw508d", "-a", "cu", "-r", "1000:2000"])
    assert "a 1... pattern needs -a c, u or cu" in refused(cli, ["add", "-p", "1Love", "-a", "e", "-r", "1000:2000"])
    assert "no address can start with it" in refused(cli, ["add", "-p", "1" * 23, "-r", "1000:2000"])
    # a file of patterns: every line is planned, the first refusal names its pattern
    f = tmp_path / "patterns.txt"
    f.write_text("1Love\n\n  1QLbz7  \n1I\n")
    assert "pattern '1I': a character outside the base58 alphabet" in refused(cli, ["add", "-p", str(f), "-r", "1000:2000"])
    f.write_text("\n\n")
    assert "no patterns in file" in refused(cli, ["add", "-p", str(f), "-r", "1000:2000"])
    for args in ([], ["-h"]):
        out = subprocess.run([cli] + args, capture_output=True, text=True, timeout=60).stdout
        assert "-p <pattern>" in out and "EIP-55 case is not matched" in out and "2^-16" in out and "bc1q" in out


def test_cli_bound_one_pattern_just_inside_and_one_just_outside(cli):
    err = refused(cli, ["add", "-p", "0xdea", "-a", "e", "-r", "1000:2000"])  # 2^-12
    assert "cover more than 2^-16" in err and "lengthen the pattern" in err and "'0xdea'" in err
    err = refused(cli, ["add", "-p", "bc1qw50", "-r", "1000:2000"])  # 2^-15: the first length above the bound
    assert "cover more than 2^-16" in err
    # 2^-16 itself passes the planner: what stops the run, if anything, is the missing GPU (or nothing: the range is 4096 keys)
    pr = subprocess.run([cli, "add", "-p", "0xdead", "-a", "e", "-r", "1000:2000"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=300)
    assert "cover more than" not in pr.stderr and "pattern '" not in pr.stderr
    assert pr.returncode == 0 or "no MI355X GPU visible" in pr.stderr


def test_binding():
    from ecloop_amd import capi
    assert capi.PREFIX == 4096 and len(capi.EXPORTS) == 45 and capi.E_NOBLOOM == -5
    text = open(os.path.join(ROOT, "include", "ecloop_hip.h")).read()
    assert "#define ECL_PREFIX 4096u" in text
    for kw in (dict(p2sh=True), dict(a33=False, tr=True), dict(a33=False, pub=True), dict(a33=False, a65=False)):
        with pytest.raises(ValueError):
            capi.Device(0, prefix=True, **kw)  # refused before the library is asked
