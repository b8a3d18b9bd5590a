"""Ethereum patterns with wildcards and suffixes (-p 0xdead*beef) on the CPU: the planner in C (ecloop_amd/host/mask_plan.h) against its
Python mirror (engine.mask_table) and both against the text yardstick tests/mask_ref.py; the routing rule (a list without ? or * is planned
as ever); the device filter csrc/mask.h compiled for the host; engine.prefix_search on a stand-in device; the CLI's refusals; and the host
program of csrc/tools/mask_host.cpp built and run under AddressSanitizer and UBSan."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import mask_ref as R
from ecloop_amd import capi, engine
from support import ROOT, cli, host_lib, host_program, run_program

E_CHAR, E_NONE, E_TYPE, E_WIDE, E_MANY = -1, -2, -3, -5, -6
D40 = "0123456789abcdef0123456789abcdef01234567"

# (pattern, digits it fixes): head only with ?, suffix only, both ends, * between parts that total 40 digits, a trailing *, upper and mixed case
GOOD = [("0xde?d", 3), ("0x?ead", 3), ("0xdead?", 4), ("0xd?a?b?e?", 4), ("0x" + "?" * 39 + "7", 1), ("0x" + D40[:39] + "?", 39),
        ("0x*beef", 4), ("0x*b", 1), ("0x*?eef", 3), ("0x*be?f", 3), ("0x*" + D40, 40), ("0x*" + "?" + D40[1:], 39),
        ("0xdead*beef", 8), ("0xd*f", 2), ("0xde?d*be?f", 6), ("0x?*?f", 1), ("0x" + D40[:20] + "*" + D40[20:], 40), ("0x" + D40[:1] + "*" + D40[1:], 40),
        ("0x" + D40[:39] + "*" + D40[39:], 40), ("0x" + D40[:17] + "*" + D40[:17], 34),
        ("0xdead*", 4), ("0xdeadbeef*", 8), ("0xde?d*", 3), ("0x" + D40 + "*", 40),
        ("0XDEAD*BEEF", 8), ("0xDeAd*bEeF", 8), ("0xDE?D", 3), ("0x*BeEf", 4),
        ("0xdeadbeef", 8), ("0x0", 1), ("0x" + D40, 40)]
# (pattern, eth, code, text of the reason)
BAD = [("0xde*ad*", True, E_CHAR, "more than one *"), ("0x**", True, E_CHAR, "more than one *"),
       ("0x?", True, E_NONE, "no hex digit at all"), ("0x*", True, E_NONE, "no hex digit at all"), ("0x??*??", True, E_NONE, "no hex digit at all"),
       ("0x" + D40 + "?", True, E_NONE, "too long"), ("0x" + D40[:20] + "*" + D40[:21], True, E_NONE, "too long"), ("0x" + "?" * 43, True, E_NONE, "empty or too long"),
       ("0xdead*beef", False, E_TYPE, "a 0x pattern needs -a e"), ("0xde?d", False, E_TYPE, "a 0x pattern needs -a e"),
       ("0xg", True, E_CHAR, "a character that is no hex digit"), ("0xde?g", True, E_CHAR, "a character that is no hex digit"),
       ("0xde d*", True, E_CHAR, "a character that is no hex digit"), ("0xdead+*", True, E_CHAR, "a character that is no hex digit"),
       ("0x", True, E_NONE, "1 ... 40 hex digits after 0x"),
       ("1Love", True, E_TYPE, "a 1... pattern needs -a c, u or cu"), ("bc1qw508", True, E_TYPE, "a bc1q pattern needs -a c"),
       ("3J98t1", True, -4, "P2SH patterns (3...) are not supported yet"), ("dead*", True, E_NONE, "patterns start with 1, bc1q or 0x")]


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    lib = host_lib(tmp_path_factory, "mask_host.cpp")
    lib.mk_test_many.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.mk_table_ok.argtypes = [C.c_void_p, C.c_ulonglong]
    lib.mk_pattern_entry.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.c_char_p]
    lib.mk_plan.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p]
    lib.mk_match.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_char_p]
    lib.mk_list_is_masked.argtypes = [C.c_char_p]
    lib.mk_sizeof_mask_t.restype = C.c_uint
    return lib


def c_entry(H, pattern, eth=True):
    """-> (code, (mask, value), digits, reason)"""
    out, digits, why = np.zeros(10, np.uint32), C.c_uint32(), C.create_string_buffer(320)
    rc = H.mk_pattern_entry(pattern.encode(), int(eth), out.ctypes.data, C.byref(digits), why)
    return rc, (R.value_of(out[:5]), R.value_of(out[5:])), digits.value, why.value.decode()


def c_plan(H, patterns, eth=True):
    """-> (entry count or code, table, entry_of, reason)"""
    table, entry_of, why = np.zeros((16, 10), np.uint32), np.zeros(max(1, len(patterns)), np.uint32), C.create_string_buffer(320)
    n = H.mk_plan("\n".join(patterns).encode(), int(eth), table.ctypes.data, entry_of.ctypes.data, why)
    return n, table[:max(n, 0)], [int(v) for v in entry_of[:len(patterns)]], why.value.decode()


# ---- the planner: C against Python, both against the text

@pytest.mark.parametrize("pattern,digits", GOOD)
def test_entry_of_a_pattern_in_c_and_python_and_by_the_text(H, pattern, digits):
    rc, (m, v), dg, why = c_entry(H, pattern)
    assert rc == 0 and dg == digits and v & ~m == 0 and bin(m).count("1") == 4 * digits, why
    assert engine.mask_pattern_entry(pattern) == (m, v, digits)  # the mirror
    # by the text: v itself matches, flipping any fixed bit does not, flipping any free bit still does
    rng = random.Random(pattern)
    free = R.TOP & ~m
    for _ in range(20):
        x = v | (rng.getrandbits(160) & free)
        assert R.matches(pattern, x) and R.has([(m, v)], x)
        bit = 1 << rng.randrange(160)
        assert R.matches(pattern, x ^ bit) == (not bit & m) == R.has([(m, v)], x ^ bit)


def test_bit_positions_of_head_and_tail_digits(H):
    # digit i from the start fixes bits 159 - 4i ... 156 - 4i, digit j from the end fixes bits 4j + 3 ... 4j
    for i in range(40):
        assert c_entry(H, "0x" + "?" * i + "a")[1] == (0xF << (156 - 4 * i), 0xA << (156 - 4 * i))
        assert c_entry(H, "0x*5" + "?" * i)[1] == (0xF << (4 * i), 0x5 << (4 * i))


@pytest.mark.parametrize("pattern,eth,code,text", BAD)
def test_refusals_name_the_pattern_in_c_and_python(H, pattern, eth, code, text):
    rc, _, _, why = c_entry(H, pattern, eth)
    assert rc == code and text in why and ("pattern '%s':" % pattern) in why
    with pytest.raises(engine.PrefixError) as e:
        engine.mask_pattern_entry(pattern, eth)
    assert str(e.value) == why  # the mirror words it the same way
    n, _, _, why2 = c_plan(H, ["0xdeadbeef*", pattern], eth)  # ... and a list with it is refused for it
    assert (n, why2) == (code, why) if eth else n == E_TYPE


def test_0xg_keeps_its_message_and_code_on_either_route(H):
    rc, _, _, why = c_entry(H, "0xg")
    assert (rc, why) == (E_CHAR, "pattern '0xg': a character that is no hex digit")
    with pytest.raises(engine.PrefixError) as e:
        engine.prefix_ranges(["0xg"], False, False, True)
    assert str(e.value) == why
    assert not engine.mask_is_masked("0xg") and not H.mk_list_is_masked(b"0xg")


def test_plan_merges_duplicates_and_keeps_list_order(H):
    patterns = ["0xdead0*", "0x*beef1", "0xDEAD0", "0xdead0*beef1", "0xDeAd0*", "0x*BEEF1", "0xd?ad00*"]
    n, table, entry_of, why = c_plan(H, patterns)
    assert n == 4 and entry_of == [0, 1, 0, 2, 0, 1, 3], why
    ptable, serves = engine.mask_table(patterns)
    assert (ptable == table).all() and serves == [[0, 2, 4], [1, 5], [3], [6]]
    assert capi_table_ok(H, table)


def capi_table_ok(H, table):
    t = np.ascontiguousarray(table, np.uint32)
    return bool(H.mk_table_ok(t.ctypes.data, len(t)))


def test_plan_bounds_sixteen_entries_and_the_coverage(H):
    five = ["0x%05x*" % (0xABC00 + i) for i in range(17)]
    n, table, _, why = c_plan(H, five[:16])  # sixteen patterns of five digits: 16 * 2^-20 = 2^-16, the bound itself
    assert n == 16 and (engine.mask_table(five[:16])[0] == table).all()
    n, _, _, why = c_plan(H, five)
    assert n == E_MANY and "more than 16 mask entries: split the list" in why and "'0xabc00*'" in why
    with pytest.raises(engine.PrefixError) as e:
        engine.mask_table(five)
    assert str(e.value) == why
    n, _, _, _ = c_plan(H, five[:16] + ["0xABC00*", "0xabc01"])  # duplicates do not count
    assert n == 16
    for patterns in (["0xdea*"], ["0x*ead"], ["0xd*ad"], ["0xdead*", "0x*beef"], ["0x????dea"], five[:15] + ["0x*abcd"], ["0xdead*", "0x" + D40 + "*"]):
        n, _, _, why = c_plan(H, patterns)
        assert n == E_WIDE and "cover more than 2^-16 of all addresses" in why and "lengthen the pattern" in why and ("'%s'" % patterns[0]) in why, patterns
        with pytest.raises(engine.PrefixError) as e:
            engine.mask_table(patterns)
        assert str(e.value) == why
    for patterns in (["0xdead*"], ["0x*dead"], ["0xde*ad"], ["0xd?e?a?d*"], ["0xdead0*", "0x*beef0", "0xde?d0*beef?"]):  # 2^-16 itself and below
        assert c_plan(H, patterns)[0] == len(patterns) == len(engine.mask_table(patterns)[0])
    assert c_plan(H, [])[0] == E_NONE
    with pytest.raises(engine.PrefixError):
        engine.mask_table([])


def test_a_list_without_wildcards_is_planned_exactly_as_before(H):
    plain = [["0xdeadbeef"], ["0xDEAD0", "0xdeae1", "0x0123456"], ["0x%040x" % 7], ["1Love"], ["1QLbz7", "bc1qw508d6"]]
    for patterns in plain:
        assert not H.mk_list_is_masked("\n".join(patterns).encode()) and not any(engine.mask_is_masked(p) for p in patterns)
    for patterns in (["0xdead*"], ["0xdeadbeef", "0xde?dbeef"], ["0x*beef0"], ["0XDEAD?"]):
        assert H.mk_list_is_masked("\n".join(patterns).encode()) and any(engine.mask_is_masked(p) for p in patterns)
    assert not engine.mask_is_masked("1Lo?e") and not H.mk_list_is_masked(b"1Lo*e\nbc1q?")  # ? and * outside 0x patterns route nothing
    # ... and prefix_search hands such a list to prefix_ranges, whose table goes to set_prefixes as it is
    seen = {}

    class Dev:
        def __init__(self, device=0, **kw):
            seen["kw"] = kw

        def set_prefixes(self, table):
            seen["table"] = np.array(table)

        def set_masks(self, table):
            raise AssertionError("a list without ? or * became a mask table")

        def geometry(self):
            return 64, 512

        def add_range(self, start, nkeys, cap=4096):
            return np.zeros(0, capi.FOUND_DTYPE), 0

        def close(self):
            pass

    for patterns in plain[:3]:
        seen.clear()
        assert engine.prefix_search(patterns, 0x8000, 0x9000, eth=True, device_cls=Dev) == ([], 0)
        table, _ = engine.prefix_ranges(patterns, False, False, True)
        assert seen["kw"].get("prefix") is True and "mask" not in seen["kw"] and seen["table"].dtype == table.dtype and (seen["table"] == table).all()
    # the wildcard refusals of the other forms stay the alphabet checks'
    for p, kw, text in (("1Lo?e", {}, "outside the base58 alphabet"), ("1Love*", {}, "outside the base58 alphabet"), ("bc1qw5?8", {}, "outside the bech32 alphabet")):
        with pytest.raises(engine.PrefixError) as e:
            engine.prefix_ranges([p], True, False, False)
        assert text in str(e.value)


# ---- the property test: membership by the table == a text match of the lower-case address

def random_pattern(rng):
    head, tail = rng.randrange(0, 12), rng.randrange(0, 12)
    style = rng.randrange(4)
    if style == 0:
        tail = 0
    elif style == 1:
        head = 0
    elif style == 3:
        head = rng.randrange(0, 41)
        tail = 40 - head if rng.random() < 0.5 else rng.randrange(0, 41 - head)
    digit = lambda: "?" if rng.random() < 0.25 else rng.choice("0123456789abcdefABCDEF")
    h, t = "".join(digit() for _ in range(head)), "".join(digit() for _ in range(tail))
    star = tail or style != 0 or rng.random() < 0.3
    return "0x" + h + ("*" + t if star else "")


def test_membership_by_table_equals_the_text_match(H):
    rng = random.Random(20260)
    checked = positive = 0
    while checked < 3000:
        p = random_pattern(rng)
        rc, (m, v), digits, _ = c_entry(H, p)
        if rc != 0:  # (nothing fixed, or nothing at all)
            with pytest.raises(engine.PrefixError):
                engine.mask_pattern_entry(p)
            continue
        assert engine.mask_pattern_entry(p) == (m, v, digits)
        for want in (True, False):  # half of the values are made to match: the pattern's own digits, anything in the free places
            x = rng.getrandbits(160)
            if want:
                d = p[2:].lower()
                head, tail = d.split("*") if "*" in d else (d, "")
                text = list("%040x" % x)
                for i, c in enumerate(head):
                    text[i] = c if c != "?" else text[i]
                for j, c in enumerate(tail):
                    text[40 - len(tail) + j] = c if c != "?" else text[40 - len(tail) + j]
                x = int("".join(text), 16)
            elif rng.random() < 0.5:  # a near miss: one fixed nibble of a matching value changed
                x = (v | x & ~m) ^ ((m & -m) * rng.randrange(1, 16))
            by_text = R.matches(p, x)
            assert by_text == R.has([(m, v)], x) == (engine.prefix_match([p], R.words5(x), "eth") is not None), (p, hex(x))
            assert not want or by_text
            hit = np.zeros(1, np.uint8)
            xs, t = np.array(R.words5(x), np.uint32), R.table_of([(m, v)])
            assert H.mk_test_many(t.ctypes.data, 1, xs.ctypes.data, 1, hit.ctypes.data) == 0 and bool(hit[0]) == by_text
            positive += by_text
            checked += 1
    assert positive >= 1500


def test_match_returns_the_first_pattern_in_list_order(H):
    v = 0x0123456789ABCDEFDEADBEEF0BADF00DFEEDFACE
    patterns = ["0xfffff*", "0x*dfacf", "0x0123?567*FACE", "0x01234*", "0x*dface"]
    addr = C.create_string_buffer(48)
    h = np.array(R.words5(v), np.uint32)
    assert H.mk_match("\n".join(patterns).encode(), 1, h.ctypes.data, addr) == 2 == R.first_match(patterns, v)
    assert addr.value.decode() == R.eth(v) == engine.prefix_match(patterns, R.words5(v), "eth")
    assert H.mk_match("\n".join(patterns[3:]).encode(), 1, h.ctypes.data, addr) == 0
    assert H.mk_match("\n".join(patterns[:2]).encode(), 1, h.ctypes.data, addr) == -1 and engine.prefix_match(patterns[:2], R.words5(v), "eth") is None
    assert engine.prefix_match(["0x0123?567*FACE"], R.words5(v), "addr33") is None  # an Ethereum pattern matches eth records only
    assert engine.prefix_match(["0x01234567"], R.words5(v), "eth") == R.eth(v) and engine.prefix_match(["0x1234567"], R.words5(v), "eth") is None


# ---- csrc/mask.h built with g++

def test_mask_filter_on_the_synthetic_cases(H):
    assert H.mk_sizeof_mask_t() == 24  # the filter field of add_args: the kernarg layout stays
    seen = set()
    for name, (entries, values) in sorted(R.mask_filter_cases().items()):
        table = R.table_of(entries)
        vals = np.array([R.words5(v) for v in values], np.uint32).reshape(-1, 5)
        hit = np.zeros(len(vals), np.uint8)
        assert H.mk_test_many(table.ctypes.data, len(table), vals.ctypes.data, len(vals), hit.ctypes.data) == 0, name
        want = R.expect(entries, values)
        assert [int(x) for x in hit] == want, name
        seen.update(want)
        if name.startswith("word"):
            w = int(name[4:])  # the hit, the value with every free bit flipped, then one flipped bit each: a miss iff the bit is fixed
            assert want[:2] == [1, 1] and want[2:] == [0 if 8 <= b < 24 else 1 for b in range(32)], name
        if name.startswith("boundary"):
            assert want == [1, 0, 0, 1], name
    assert R.expect(*R.mask_filter_cases()["zero_mask"]) == [1, 1, 1]
    assert R.expect(*R.mask_filter_cases()["last_of_16"]) == [1, 0, 0] + [1] * 15
    assert seen == {0, 1}


def test_table_check_refusals(H):
    ok = lambda entries, n=None: bool(H.mk_table_ok(R.table_of(entries).ctypes.data, len(entries) if n is None else n))
    good = [(R.FULL, i) for i in range(17)]
    assert ok(good[:1]) and ok(good[:16]) and ok([(0, 0)]) and ok([(0, 0), (0xF << 156, 0)])
    assert not ok(good[:1], 0) and not ok(good, 17)
    for w in range(5):
        assert not ok([(0xFF00 << (32 * w), 0x1 << (32 * w))])  # a value bit outside the mask, in each word
        assert not ok([(1 << (32 * w), 0)] * 2) and not ok(good[:3] + [(1 << (32 * w), 0)] + good[3:9] + [(1 << (32 * w), 0)])  # the same entry twice
    assert ok([(0xF, 1), (0xF, 2)]) and ok([(0xF, 1), (0xFF, 1)])  # the same value under two masks, two values under one: distinct
    hit = np.zeros(1, np.uint8)
    t, x = R.table_of([(0xF, 0x10)]), np.zeros(5, np.uint32)
    assert H.mk_test_many(t.ctypes.data, 1, x.ctypes.data, 1, hit.ctypes.data) == -1


# ---- engine.prefix_search on the stand-in device

START, NKEYS = 0x8000, 2048  # (one group of cmd_add's job arithmetic)


@pytest.fixture(scope="module")
def addresses():
    """the address of every key x image of the range, by tests/eth_ref.py"""
    import orc
    return {(off, e): R.value_of(R.eth_words_of(*engine.splitkey_image_origin(orc.point_of(START + off), e))) for off in range(NKEYS) for e in range(6)}


@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
def test_prefix_search_with_masked_patterns(addresses, endo):
    a, b, c = R.eth(addresses[(17, 0)]), R.eth(addresses[(200, 0)]), R.eth(addresses[(99, 4 if endo else 0)])
    patterns = [a[:4] + "*" + a[-3:], b[:4].upper().replace("0X", "0x") + "?" + b[5:8], "0x*" + c[-5:], a[:4] + "*" + a[-3:].upper()]
    want = {}
    for (off, e), v in addresses.items():
        if (endo or e == 0) and R.first_match(patterns, v) is not None:
            want[("eth", v, engine.calc_priv(START, 1, off, e))] = R.eth(v)
    assert len(want) >= 3
    R.FakeMaskDevice.tables.clear(), R.FakeMaskDevice.opened.clear()
    found, edge = engine.prefix_search(patterns, START, START + NKEYS, eth=True, endo=endo, device_cls=R.FakeMaskDevice)
    assert {(f.label, R.value_of(f.h160), f.pk): f.address for f in found} == want and len(found) == len(want) and edge == 0
    table, serves = engine.mask_table(patterns)
    assert len(table) == 3 and serves[0] == [0, 3]  # the duplicate merged
    assert len(R.FakeMaskDevice.tables) == 1 and (R.FakeMaskDevice.tables[0] == table).all() and R.FakeMaskDevice.opened == [dict(endo=endo, origin=False)]
    f = found[0]
    assert f.stdout_line() == "eth: %040x <- %064x %s" % (R.value_of(f.h160), f.pk, f.address)


def test_prefix_search_with_masked_patterns_from_an_origin(addresses):
    import eth_ref
    import orc
    kq = 0x1234567
    Q = orc.point_of(kq)
    k = 77
    addr = R.eth(R.value_of(eth_ref.eth_words(*orc.point_of(kq + START + k))))
    pattern = addr[:4] + "*" + addr[-4:]
    R.FakeMaskDevice.opened.clear()
    found, edge = engine.prefix_search([pattern], START, START + NKEYS, eth=True, device_cls=R.FakeMaskDevice, origin=Q)
    assert edge == 0 and R.FakeMaskDevice.opened == [dict(endo=False, origin=True)]
    hit = [f for f in found if f.pk == START + k]
    assert len(hit) == 1 and hit[0].split == 0 and hit[0].address == addr
    final = engine.splitkey_combine(kq, hit[0].pk, hit[0].split)
    assert R.eth(R.value_of(eth_ref.eth_words(*orc.point_of(final)))) == addr and R.matches(pattern, int(addr, 16))


def test_a_record_that_matches_no_pattern_is_an_error_not_an_edge(addresses):
    class Liar(R.FakeMaskDevice):
        def set_masks(self, table):
            super().set_masks(table)
            self.entries = [(0, 0)]  # reports every key

    a = R.eth(addresses[(5, 0)])
    with pytest.raises(engine.EclError) as e:
        engine.prefix_search([a[:6] + "*" + a[-2:]], START, START + 16, eth=True, device_cls=Liar)
    assert "matches no pattern" in str(e.value)


def test_refused_masked_patterns_reach_no_device():
    class Never:
        def __init__(self, *a, **k):
            raise AssertionError("opened a device for a refused pattern")
    for patterns, kw in ((["0xde*"], dict(eth=True)), (["0xdead*beef"], {}), (["0xdead*be*ef"], dict(eth=True)), (["0x?*"], dict(eth=True)),
                         (["0xdead0*", "1Love"], dict(eth=True)), (["0x%05x*" % i for i in range(17)], dict(eth=True))):
        with pytest.raises(engine.PrefixError):
            engine.prefix_search(patterns, 0x8000, 0x9000, device_cls=Never, **kw)


def test_binding():
    assert capi.MASK == 8192 and len(capi.EXPORTS) == 45
    text = open(os.path.join(ROOT, "include", "ecloop_hip.h")).read()
    assert "#define ECL_MASK 0x2000u" in text and 0x2000 == capi.MASK
    for kw in (dict(a33=True, eth=False), dict(a33=False, eth=True, prefix=True), dict(a33=False, eth=True, p2sh=True), dict(a33=False, eth=False, pub=True),
               dict(a33=False, eth=False, tr=True), dict(a33=False, a65=True, eth=False)):
        with pytest.raises(ValueError):
            capi.Device(0, mask=True, **kw)  # refused before the library is asked


# ---- the CLI (no GPU is reached: everything here is decided before a device is opened)

def refused(cli, args):
    pr = subprocess.run([cli] + args, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=120)
    assert pr.returncode == 1, (args, pr.stdout, pr.stderr)
    return pr.stderr


def test_cli_refusals_and_help(cli, tmp_path):
    tail = ["-a", "e", "-r", "8000:8fff"]
    assert "pattern '0xde*ad*': more than one *" in refused(cli, ["add", "-p", "0xde*ad*"] + tail)
    assert "pattern '0x?*': no hex digit at all" in refused(cli, ["rnd", "-p", "0x?*", "-a", "e"])
    assert "pattern '0x" + D40 + "?': no address can match it (too long" in refused(cli, ["add", "-p", "0x" + D40 + "?"] + tail)
    assert "pattern '0xdead*beef': a 0x pattern needs -a e" in refused(cli, ["add", "-p", "0xdead*beef", "-r", "8000:8fff"])
    assert "pattern '0xg': a character that is no hex digit" in refused(cli, ["add", "-p", "0xg"] + tail)
    assert "pattern '0xde?g': a character that is no hex digit" in refused(cli, ["add", "-p", "0xde?g"] + tail)
    err = refused(cli, ["add", "-p", "0xde*"] + tail)
    assert "cover more than 2^-16" in err and "lengthen the pattern" in err and "'0xde*'" in err
    assert "-p and -f exclude each other" in refused(cli, ["add", "-p", "0xdead*beef", "-f", "x.blf"] + tail)
    assert "-p is not supported with mul" in refused(cli, ["mul", "-p", "0xdead*beef", "-a", "e"])
    for a in ("s", "t", "x"):
        assert "-p is not supported with -a %s" % a in refused(cli, ["add", "-p", "0xdead*beef", "-a", a, "-r", "8000:8fff"])
    assert "outside the base58 alphabet" in refused(cli, ["add", "-p", "1Lo?e", "-r", "8000:8fff"])
    assert "outside the bech32 alphabet" in refused(cli, ["add", "-p", "bc1qw5*8", "-r", "8000:8fff"])
    f = tmp_path / "patterns.txt"
    f.write_text("".join("0x%05x*\n" % (0xABC00 + i) for i in range(17)))
    assert "more than 16 mask entries: split the list" in refused(cli, ["add", "-p", str(f)] + tail)
    f.write_text("0xdead0*\n\n  0x*beef0  \n0xdead*be*ef\n")
    assert "pattern '0xdead*be*ef': more than one *" in refused(cli, ["add", "-p", str(f)] + tail)
    # a list that passes the planner: what stops the run, if anything, is the missing GPU
    f.write_text("0xdead0*\n0x*beef0\n0xde?d00\n")
    pr = subprocess.run([cli, "add", "-p", str(f)] + tail, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=300)
    assert "pattern '" not in pr.stderr and "cover more than" not in pr.stderr
    assert pr.returncode == 0 or "no MI355X GPU visible" in pr.stderr
    out = subprocess.run([cli, "-h"], capture_output=True, text=True, timeout=60).stdout
    assert "'0xdead*beef'" in out and "in quotes" in out and "at most 16" in out


# ---- the host program under the sanitizers: built with its own main and run directly

def test_host_program_under_asan_and_ubsan(tmp_path):
    pr = run_program(host_program(tmp_path, "mask_host.cpp", ["-O1", "-g"]))
    assert pr.returncode == 0 and pr.stdout.strip() == "ok", (pr.stdout, pr.stderr[-2000:])
