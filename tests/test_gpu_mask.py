"""Ethereum patterns with wildcards and suffixes (-p 0xdead*beef, ECL_MASK) on the GPU: the mask kernels' records against the yardstick's
addresses (tests/eth_ref.py through test_gpu_prefix.eth_records) and a table built from them, dense hits through the ring, keys past nkeys,
split and strided calls, ecl_hip_diag_bloom against the host build of mask.h, the ABI's refusals, the split-key walk, and the CLI's found
lines against the text yardstick tests/mask_ref.py.  Every GPU-using subprocess runs under its own time limit."""
import ctypes as C

import numpy as np
import pytest

import eth_ref
import mask_ref as R
import orc
from support import cli, host_lib, run_cli
from test_gpu_prefix import NKEYS, START, eth_records

pytestmark = pytest.mark.gpu
TYPES = {"e": dict(endo=False), "e-endo": dict(endo=True)}
ZERO = [(0, 0)]


def records(name):
    return [r for r in eth_records() if TYPES[name]["endo"] or r[2] == 0]


def keys_of(recs):
    return sorted((int(r["key_offset"]), tuple(int(w) for w in r["h160"]), int(r["endo"]), int(r["compressed"])) for r in recs)


def open_mask(name="e", geometry=None, offs=0, origin=False):
    from ecloop_amd import Device
    d = Device(0, a33=False, eth=True, mask=True, ord_offs=offs, origin=origin, **TYPES[name])
    if geometry:
        d.set_geometry(*geometry)
    return d


def sixteen_entries(recs):
    """five entries fixing 16 bits of one word each, one full 160-bit entry, five full-width near misses (a real address with one bit
    flipped, one per word), five head + tail entries (the leading and the last four bits) -> (entries, near-miss values)"""
    vals = [R.value_of(r[1]) for r in recs]
    pick = lambda i: vals[(len(vals) * (2 * i + 1)) // 40]  # twenty records spread over the set
    entries = []
    for w in range(5):
        m = 0x00FFFF00 << (32 * (4 - w))
        entries.append((m, pick(w) & m))
    entries.append((R.FULL, pick(5)))
    near = [pick(6 + w) ^ (1 << (32 * (4 - w) + 7 * w + 1)) for w in range(5)]
    entries += [(R.FULL, v) for v in near]
    m = 0xF << 156 | 0xF
    entries += [(m, pick(11 + i) & m) for i in range(5)]
    assert len(entries) == 16 and len(set(entries)) == 16
    return entries, near


@pytest.mark.parametrize("geometry", [(8, 256), None], ids=["8x256", "auto"])
@pytest.mark.parametrize("name", list(TYPES))
def test_exact_set_parity(name, geometry):
    all_recs = records(name)
    entries, near = sixteen_entries(all_recs)
    want = sorted(r for r in all_recs if R.has(entries, R.value_of(r[1])))
    present = {R.value_of(r[1]) for r in all_recs}
    assert 10 <= len(want) <= len(all_recs) // 10 and not any(v in present for v in near)
    d = open_mask(name, geometry)
    try:
        d.set_masks(R.table_of(entries))
        before = d.coverage()
        recs, total = d.add_range(START, NKEYS, cap=4096)
        after = d.coverage()
    finally:
        d.close()
    got = keys_of(recs)
    assert total == len(recs) and len(got) == len(set(got))  # no duplicates
    assert got == want  # no false positive, nothing missed, the near misses stay out
    assert tuple(b - a for a, b in zip(before, after)) == (NKEYS, NKEYS, NKEYS)  # requested == covered == counted on the device


@pytest.mark.parametrize("name", list(TYPES))
def test_dense_hits_once_per_key_and_image_and_overflow_keeps_the_rest(name):
    want = sorted(records(name))
    table = R.table_of([(0, 0), (0xF << 156, 0)])  # everything matches the first entry, a sixteenth of it the second one as well
    assert sum(1 for r in want if r[1][0] >> 28 == 0) > 100
    d = open_mask(name, (8, 256))
    try:
        d.set_masks(table)
        recs, total = d.add_range(START, NKEYS, cap=len(want) + 16)
        assert total == len(recs) == len(want) and keys_of(recs) == want  # every key, every image, once
        first, total = d.add_range(START, NKEYS, cap=16)  # ECL_E_OVERFLOW: the true total, sixteen records, the rest still on the device
        assert total == len(want) and len(first) == 16
        rest = d.fetch_found(16, total - 16)
        assert len(rest) == total - 16 and keys_of(np.concatenate([first, rest])) == want
    finally:
        d.close()


def test_no_record_past_nkeys():
    want = sorted(r for r in records("e-endo") if r[0] < 1000)
    for geometry in ((8, 256), None):
        d = open_mask("e-endo", geometry)
        try:
            d.set_masks(R.table_of(ZERO))
            recs, total = d.add_range(START, 1000, cap=6000)
            assert total == len(recs) == 6000 and max(int(r["key_offset"]) for r in recs) == 999 and keys_of(recs) == want
            assert d.coverage() == (1000, 1000, 1000)
        finally:
            d.close()


def test_split_calls_and_a_strided_call():
    all_recs = records("e-endo")
    entries, _ = sixteen_entries(all_recs)
    want = sorted(r for r in all_recs if R.has(entries, R.value_of(r[1])))
    d = open_mask("e-endo", (8, 256))
    try:
        d.set_masks(R.table_of(entries))
        one, _ = d.add_range(START, NKEYS)
        a, _ = d.add_range(START, 2048)
        b, _ = d.add_range(START + 2048, 2048)  # contiguous: continues the resident walk
        b = b.copy()
        b["key_offset"] += 2048
        assert keys_of(np.concatenate([a, b])) == keys_of(one) == want
        assert len(a) and len(b)
    finally:
        d.close()
    start = 0x123456789ABCDEF
    strided = [(off, R.eth_words_of(*orc.point_of(start + (off << 12))), 0, 3) for off in range(2048)]
    m = 0xF << 156 | 0xF
    entries = [(m, R.value_of(strided[100 * i + 7][1]) & m) for i in range(1, 9)]
    entries = sorted(set(entries))
    want = sorted(r for r in strided if R.has(entries, R.value_of(r[1])))
    assert len(want) >= 20
    d = open_mask("e", offs=12)
    try:
        d.set_masks(R.table_of(entries))
        recs, total = d.add_range(start, 2048)
        assert total == len(recs) and keys_of(recs) == want
    finally:
        d.close()


def test_diag_bloom_runs_the_mask_test(tmp_path_factory):
    """the synthetic cases of the CPU test (tests/mask_ref.py: mask_filter_cases): the device's answers equal the host build's"""
    H = host_lib(tmp_path_factory, "mask_host.cpp")
    H.mk_test_many.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    d = open_mask("e")
    try:
        answers = set()
        for name, (entries, values) in sorted(R.mask_filter_cases().items()):
            table = R.table_of(entries)
            vals = np.array([R.words5(v) for v in values], np.uint32).reshape(-1, 5)
            host = np.zeros(len(vals), np.uint8)
            assert H.mk_test_many(table.ctypes.data, len(table), vals.ctypes.data, len(vals), host.ctypes.data) == 0
            d.set_masks(table)
            dev = d.diag_bloom(vals)
            assert (dev == host).all(), name
            assert [int(v) for v in dev] == R.expect(entries, values), name
            answers.update(int(v) for v in dev)
        assert answers == {0, 1}
    finally:
        d.close()


def test_abi_refusals_and_acceptances():
    from ecloop_amd import capi
    lib = capi.load()
    M, E = capi.MASK, capi.ETH
    bad = [M, M | capi.ENDO, M | capi.ADDR33, M | capi.ADDR65 | capi.ENDO, M | E | capi.ADDR33, M | E | capi.PREFIX, M | capi.PREFIX | capi.ADDR33,
           capi.PREFIX | capi.ORIGIN | capi.ADDR33 | M, M | E | capi.P2SH, M | capi.TR, M | E | capi.TR, M | capi.PUB, M | E | capi.PUB, M | capi.PUB | capi.ORIGIN,
           M | E | capi.INSERT, M | capi.PUB | capi.INSERT, M | E | capi.HERD, M | capi.PUB | capi.HERD, M | capi.ORIGIN, M | E | 8, M | E | 32, M | E | 16384]
    for flags in bad:
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, flags, 0) == capi.E_ARG, flags
    for flags in (M | E, M | E | capi.ENDO, M | E | capi.ORIGIN, M | E | capi.ENDO | capi.ORIGIN):
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, flags, 0) == 0, flags  # (the self-test of the context runs the mask kernel)
        lib.ecl_hip_close(h)
    h = C.c_void_p()
    assert lib.ecl_hip_open(C.byref(h), 0, M | E, 0) == 0
    try:
        out, n = np.zeros(16, capi.FOUND_DTYPE), C.c_uint32()
        start = capi.limbs(START)
        add = lambda: lib.ecl_hip_add_range(h, start.ctypes.data, 2048, out.ctypes.data, 16, C.byref(n))
        assert add() == capi.E_NOBLOOM  # no table yet
        set_table = lambda tab, nwords: lib.ecl_hip_set_bloom(h, tab.ctypes.data, nwords)  # (tab: C-contiguous, alive in the caller)
        good = R.table_of([(R.FULL, 5), (R.FULL, 9)])
        assert set_table(good, 10) == 0 and add() == 0 and n.value == 0
        assert set_table(good, 7) == capi.E_ARG  # no multiple of 5
        assert add() == capi.E_NOBLOOM  # a refused table leaves the context without one
        assert set_table(good, 9) == capi.E_ARG and set_table(good, 0) == capi.E_ARG  # n = 0
        seventeen = R.table_of([(R.FULL, i) for i in range(17)])
        assert set_table(seventeen, 5 * 17) == capi.E_ARG  # n = 17
        assert b"mask table" in lib.ecl_hip_last_error(h)
        for w in range(5):
            assert set_table(R.table_of([(0xFF00 << (32 * w), 1 << (32 * w))]), 5) == capi.E_ARG  # a value bit outside the mask
        assert set_table(R.table_of([(R.FULL, 5), (0xF, 1), (R.FULL, 5)]), 15) == capi.E_ARG  # the same entry twice
        assert add() == capi.E_NOBLOOM
        assert set_table(seventeen, 5 * 16) == 0 and set_table(good, 10) == 0
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
        assert lib.ecl_hip_selftest(h) == 0 and add() == 0  # the self-test runs on a table of its own and puts the caller's back
    finally:
        lib.ecl_hip_close(h)


# ---- split key: the mask walk from an origin

KQ = 0x3B6F1D9A2C4E8071_95D3A7F20B1C6E48_D27A90C3F15B8E64_0A7C3E912D5F8B46  # the requester's key; Q = KQ G is all the searcher sees


def test_split_key_walk_partial_keys_and_verify():
    from ecloop_amd.engine import N, calc_priv, splitkey_combine, splitkey_image_origin
    Q = orc.point_of(KQ)
    k = START + 1234
    addr = R.value_of(eth_ref.eth_words(*orc.point_of((KQ + k) % N)))  # the address of Q + k G, by its key
    image = R.value_of(eth_ref.eth_words(*orc.point_of(calc_priv((KQ + START + 77) % N, 1, 0, 3))))  # ... and of image 3 of another point
    m = R.FULL & ~(0xFFFF << 64)
    entries = [(m, addr & m), (m, image & m)]  # 0x<head>*<tail> with a hole of four digits
    d = open_mask("e-endo", (8, 256), origin=True)
    try:
        d.set_masks(R.table_of(entries))
        recs, total = d.add_range(START, NKEYS, cap=64, origin=Q)
        assert total == len(recs) == 2
        by_off = {int(r["key_offset"]): r for r in recs}
        assert sorted(by_off) == [77, 1234]
        for off, e, v in ((1234, 0, addr), (77, 3, image)):
            r = by_off[off]
            assert int(r["endo"]) == e and int(r["compressed"]) == 3 and R.value_of(r["h160"]) == v
            partial = calc_priv(START, 1, off, e)
            final = splitkey_combine(KQ, partial, e)  # only Q's owner can form it
            assert R.value_of(eth_ref.eth_words(*orc.point_of(final))) == v
            got, ok = d.verify_eth([partial], origin=[splitkey_image_origin(Q, e)])  # re-derived by a path that is not the walk
            assert ok[0] == 1 and R.value_of(got[0]) == v
        with pytest.raises(ValueError):
            d.verify_eth([1])  # twelve limbs per entry on this context
    finally:
        d.close()


def test_engine_prefix_search_masked_with_and_without_an_origin():
    from ecloop_amd.engine import N, prefix_search, splitkey_combine
    recs = records("e")
    a, b = R.eth(R.value_of(recs[321][1])), R.eth(R.value_of(recs[3000][1]))
    patterns = [a[:5] + "*" + a[-4:], "0x*" + b[-6:].upper()]
    want = sorted((START + r[0], R.eth(R.value_of(r[1]))) for r in recs if R.first_match(patterns, R.value_of(r[1])) is not None)
    assert len(want) >= 2
    found, edge = prefix_search(patterns, START, START + NKEYS, eth=True)
    assert edge == 0 and sorted((f.pk, f.address) for f in found) == want and all(f.label == "eth" for f in found)
    # from an origin: the pattern from the address of Q + k G
    k = START + 99
    addr = R.eth(R.value_of(eth_ref.eth_words(*orc.point_of((KQ + k) % N))))
    found, edge = prefix_search([addr[:6] + "??" + addr[8:12] + "*" + addr[-6:]], START, START + 2048, eth=True, origin=orc.point_of(KQ))
    assert edge == 0 and [(f.pk, f.split, f.address) for f in found] == [(k, 0, addr)]
    assert R.eth(R.value_of(eth_ref.eth_words(*orc.point_of(splitkey_combine(KQ, found[0].pk, found[0].split))))) == addr


# ---- the CLI

def patterns_from(values):
    """three patterns cut from real addresses: head 2 + * + tail 3, a ? hole, and a pure suffix of 5"""
    a, b, c = (R.eth(v) for v in values)
    return [a[:4] + "*" + a[-3:], b[:5] + "?" + b[6:8].upper(), "0x*" + c[-5:]]


def test_cli_add_prints_the_lines_the_yardstick_expects(cli, tmp_path):
    from ecloop_amd.engine import calc_priv
    f = tmp_path / "patterns.txt"
    for name, extra in (("e", []), ("e-endo", ["-endo"])):
        recs = records(name)
        patterns = patterns_from([R.value_of(recs[i][1]) for i in (len(recs) // 7, len(recs) // 2, len(recs) - 50)])
        f.write_text("\n".join(patterns) + "\n")
        want = sorted("eth: %040x <- %064x %s" % (R.value_of(r[1]), calc_priv(START, 1, r[0], r[2]), R.eth(R.value_of(r[1])))
                      for r in recs if R.first_match(patterns, R.value_of(r[1])) is not None)
        assert len(want) >= 3
        outfile = tmp_path / ("found-%s.txt" % name)
        r = run_cli(cli, ["add", "-p", str(f), "-a", "e", "-r", "%x:%x" % (START, START + NKEYS - 1), "-o", str(outfile)] + extra, timeout=300)
        assert r.found == want, (r.stdout, r.status)
        assert "~ eth: 1 | filter: prefix (3 patterns, 3 mask entries)" in r.stdout and "edge: 0" in r.status
        assert sorted(outfile.read_text().splitlines()) == sorted(l.replace("eth: ", "eth\t").replace(" <- ", "\t").replace(" 0x", "\t0x") for l in want)


def test_cli_add_split_key(cli, tmp_path):
    from ecloop_amd.engine import N, splitkey_combine
    Q = orc.point_of(KQ)
    addr = {k: R.value_of(R.eth_words_of(*R._add(Q, orc.point_of(k)))) for k in range(START, START + NKEYS)}
    assert addr[START + 5] == R.value_of(eth_ref.eth_words(*orc.point_of((KQ + START + 5) % N)))
    patterns = patterns_from([addr[START + 300], addr[START + 2000], addr[START + 4000]])
    f = tmp_path / "patterns.txt"
    f.write_text("\n".join(patterns) + "\n")
    want = sorted("eth: %040x <- %064x %s split:0" % (v, k, R.eth(v)) for k, v in addr.items() if R.first_match(patterns, v) is not None)
    assert len(want) >= 3
    pub = "%02x%064x" % (2 | Q[1] & 1, Q[0])
    r = run_cli(cli, ["add", "-p", str(f), "-k", pub, "-a", "e", "-r", "%x:%x" % (START, START + NKEYS - 1)], timeout=300)
    assert r.found == want and "PARTIAL keys for %s" % pub in r.stdout and "edge: 0" in r.status, (r.stdout, r.status)
    for line in r.found:  # the partial key, combined with k_Q, is the key of the printed address
        _, h, _, part, a, sp = line.split()
        final = splitkey_combine(KQ, int(part, 16), int(sp.split(":")[1]))
        assert R.eth(R.value_of(eth_ref.eth_words(*orc.point_of(final)))) == a == "0x" + h


def test_cli_rnd_searches_the_window_it_prints(cli, tmp_path):
    recs = records("e")
    patterns = patterns_from([R.value_of(recs[i][1]) for i in (500, 2000, 3500)])
    f = tmp_path / "patterns.txt"
    f.write_text("\n".join(patterns) + "\n")
    inside = sorted("eth: %040x <- %064x %s" % (R.value_of(r[1]), START + r[0], R.eth(R.value_of(r[1]))) for r in recs if R.first_match(patterns, R.value_of(r[1])) is not None)
    assert len(inside) >= 3
    r = run_cli(cli, ["rnd", "-p", str(f), "-a", "e", "-seed", "mask", "-r", "%x:%x" % (START, START + NKEYS - 1), "-d", "0:20"],
                env={"ECLOOP_HIP_RND_WINDOWS": "1"}, timeout=300)
    out = r.stdout
    bounds = [int(l.replace(" ", ""), 16) for l in out.splitlines() if len(l.replace(" ", "")) == 64 and set(l) <= set("0123456789abcdef ")]
    assert bounds[:2] == [START, START + NKEYS - 1], out  # the window it prints: bits 0 ... 19 cleared / set, clamped to the range
    assert set(inside) <= set(r.found), (out, r.status)  # (rnd walks full-size jobs: 2^21 keys from the window's first key)
    for line in r.found:  # every line is a key of the walk with its own address, and the address matches a pattern
        _, h, _, k, a = line.split()
        assert START <= int(k, 16) < START + (1 << 21)
        assert R.eth(R.value_of(eth_ref.eth_words(*orc.point_of(int(k, 16))))) == a == "0x" + h and R.first_match(patterns, int(h, 16)) is not None
