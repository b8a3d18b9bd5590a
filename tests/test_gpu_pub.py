"""Public keys by x (`-a x`, ECL_PUB) on the GPU: the flag rules through the C ABI, every key of two ranges through an all-ones filter
against tests/pub_ref.py (pure Python over the oracle's points), with and without the endomorphism, geometries that must not change a
record, a sparse filter whose chance hits are the yardstick's too, overflow and fetch, list mode, the coverage check, the look-ahead,
`mul` / `mul -raw`, a full-size call against its parts, and the CLI's found lines.  Every GPU-using subprocess runs under its own time
limit."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import orc
import pub_ref
from support import GOLD, cli, counts, rec_set, run_cli
from synth import synth_bloom_words

pytestmark = pytest.mark.gpu
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
RANGES = [(0x3F000, 3000, 0), (0x123456789ABCDEF, 1500, 7)]  # the ranges of tests/test_gpu_tr.py
h160_of = pub_ref.h160_of


def pub_device(words=ONES, offs=0, lookahead=0, endo=False):
    from ecloop_amd import Device
    d = Device(0, a33=False, pub=True, endo=endo, ord_offs=offs)
    d.set_bloom(words)
    d.set_lookahead(lookahead)
    return d


def test_flags_and_verify_pub():
    from ecloop_amd import Device, capi
    lib = capi.load()
    for other in (1, 2, 8, 16, 32, 64, 128):
        for endo in (0, capi.ENDO):
            h = C.c_void_p()
            assert lib.ecl_hip_open(C.byref(h), 0, capi.PUB | other | endo, 0) == -1, other  # ECL_E_ARG: searched alone; 8 and 32 unknown
    for flags in (capi.PUB, capi.PUB | capi.ENDO):  # (each runs the self-test: its walk against the double-and-add kernel's x)
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, flags, 0) == 0, flags
        lib.ecl_hip_close(h)
    d = Device(0)  # any context can be asked
    try:
        ks = [1, 2, 0xdc2a04, orc.N - 1, 0, orc.N]
        x, par, ok = d.verify_pub(ks)
        assert [int(v) for v in ok] == [1, 1, 1, 1, 0, 0]
        for i, k in enumerate(ks[:4]):
            px, py = orc.point_of(k)
            assert sum(int(w) << (32 * (7 - j)) for j, w in enumerate(x[i])) == px and int(par[i]) == py & 1
    finally:
        d.close()


@pytest.mark.parametrize("start,nkeys,offs", RANGES, ids=["contiguous", "stride128"])
def test_every_key_once_with_the_right_x(start, nkeys, offs):
    """all-ones filter: exactly one record per key, type 5, endo 0, h160 = the leading 20 bytes of the yardstick's x; all three coverage
    totals grow by the keys asked.  With the endomorphism: three records per key, endo 0, 2, 4, and the key calc_priv gives for each
    re-derives to an x with those 20 bytes"""
    d = pub_device(offs=offs)
    try:
        before = d.coverage()
        recs, n = d.add_range(start, nkeys, cap=nkeys + 16)
        grown = tuple(b - a for a, b in zip(before, d.coverage()))
    finally:
        d.close()
    assert n == len(recs) == nkeys and sorted(int(r["key_offset"]) for r in recs) == list(range(nkeys))
    assert all(int(r["compressed"]) == 5 and int(r["endo"]) == 0 for r in recs)
    assert grown == (nkeys, nkeys, nkeys)
    for r in recs:
        k = (start + (int(r["key_offset"]) << offs)) % orc.N
        assert tuple(int(v) for v in r["h160"]) == h160_of(k), int(r["key_offset"])
    d = pub_device(offs=offs, endo=True)
    try:
        before = d.coverage()
        recs, n = d.add_range(start, nkeys, cap=3 * nkeys + 16)
        grown = tuple(b - a for a, b in zip(before, d.coverage()))
    finally:
        d.close()
    assert n == len(recs) == 3 * nkeys and grown == (nkeys, nkeys, nkeys)
    assert sorted((int(r["key_offset"]), int(r["endo"])) for r in recs) == [(i, e) for i in range(nkeys) for e in (0, 2, 4)]
    assert all(int(r["compressed"]) == 5 for r in recs)
    for r in recs[:: max(1, len(recs) // 900)]:
        k = (start + (int(r["key_offset"]) << offs)) % orc.N
        h = tuple(int(v) for v in r["h160"])
        assert h == pub_ref.endo_images(k)[int(r["endo"])]
        assert h == h160_of(pub_ref.calc_priv(k, int(r["endo"]))), (int(r["key_offset"]), int(r["endo"]))  # the host's existing calc_priv


def test_geometries_change_no_record():
    """half group 2, a ragged key count, a start that puts lane 3's centre on the jump point (the next centre by the tangent), a larger
    half group and the automatic geometry: the same records for the same keys, each the yardstick's"""
    B, T = 8, 256
    tangent = (2 * (T - 3) - 1) * B  # start + B + 3 * 2B == T * 2B (tests/test_gpu_add.py)
    nkeys = 2 * B * T * 2 + 77  # two groups per lane and a ragged rest
    want = None
    for endo in (False, True):
        sets = []
        for geo in ((8, 256), (2, 256), (64, 512), (1024, 256), None):
            d = pub_device(endo=endo)
            try:
                if geo:
                    d.set_geometry(*geo)
                recs, n = d.add_range(tangent, nkeys, cap=3 * nkeys + 16)
                assert n == len(recs) == nkeys * (3 if endo else 1), (geo, n)
                sets.append(rec_set(recs))
            finally:
                d.close()
        assert all(s == sets[0] for s in sets[1:]), endo
        if not endo:
            want = sets[0]
            assert [x[3] for x in want[:: 97]] == [h160_of(tangent + x[0]) for x in want[:: 97]]
            # the keys around the jump of lane 3 (second group of that lane: the centre that came from the tangent)
            second = 2 * B * T + 3 * 2 * B
            for x in want[second : second + 2 * B]:
                assert x[3] == h160_of(tangent + x[0]), x[0]
        else:
            assert [x for x in sets[0] if x[1] == 0] == want


def test_sparse_filter_chance_hits_and_the_negative_of_a_planted_key():
    """a filter of bit density 0.75 and 3 ... 20 probes per hash that also holds x of keys in the range and x of (n - k) G for others: the
    records - chance hits included - equal the yardstick's filter test over EVERY key of the range; a planted negative reports the walked
    key k"""
    A, nkeys = 0x5_0000_0000, 40000
    planted, negs = [0, 1, 777, 20000, nkeys - 1], [5, 12345, 39998]
    d = pub_device(synth_bloom_words(4099, 3, "a|b"))
    try:
        d.bloom_insert(np.array([list(h160_of(A + o)) for o in planted] + [list(pub_ref.words5(orc.point_of(orc.N - (A + o))[0])) for o in negs], np.uint32))
        words = d.get_bloom(4099)
        recs, n = d.add_range(A, nkeys, cap=1 << 15)
        assert n == len(recs)
    finally:
        d.close()
    flt = orc.OrcFilter(bloom_words=words)
    hs = [h160_of(A + o) for o in range(nkeys)]
    want = sorted((o, 0, 5, h) for o, h in enumerate(hs) if flt.check(list(h)))
    assert rec_set(recs) == want
    assert set(planted + negs) <= {x[0] for x in want} and len(want) > len(planted) + len(negs) + 20  # the chance hits were there to be checked


def test_overflow_delivers_the_first_records_and_fetch_the_rest():
    d = pub_device()
    try:
        recs, total = d.add_range(0x3F000, 5000, cap=100)
        rest = d.fetch_found(100, 4900)
    finally:
        d.close()
    offs = sorted([int(r["key_offset"]) for r in recs] + [int(r["key_offset"]) for r in rest])
    assert total == 5000 and len(recs) == 100 and len(rest) == 4900 and offs == list(range(5000))
    assert all(int(r["compressed"]) == 5 for r in rest)
    for r in list(recs[:5]) + list(rest[-5:]):
        assert tuple(int(v) for v in r["h160"]) == h160_of(0x3F000 + int(r["key_offset"]))


def test_list_mode_reports_exactly_the_listed_keys():
    start, nkeys = RANGES[0][0], RANGES[0][1]
    listed = sorted(random.Random(5).sample(range(nkeys), 50))
    hs = np.array(sorted(h160_of(start + off) for off in listed), np.uint32)
    d = pub_device()
    try:
        d.set_list(hs)
        recs, n = d.add_range(start, nkeys, cap=4096)
    finally:
        d.close()
    assert n == len(recs) == 50 and sorted(int(r["key_offset"]) for r in recs) == listed
    assert all(tuple(int(v) for v in r["h160"]) == h160_of(start + int(r["key_offset"])) for r in recs)


def test_mul_batch_and_mul_batch_raw_against_the_yardstick():
    """2^16 + 77 seeded random scalars plus 0, n, n - 1, 1 and short scalars, and pass phrases of 1 ... 70 bytes, all-ones filter: one
    record per scalar that is not 0 (mod n), each the yardstick's; coverage counts every scalar (0 and n are counted and not probed)"""
    rnd = random.Random(350)
    ks = [rnd.getrandbits(256) for _ in range((1 << 16) + 77)] + [0, orc.N, orc.N - 1, 1, 2, 0xFFFF, 1 << 64, (1 << 128) + 3, 2 * orc.N]
    ks = [k % (1 << 256) for k in ks]
    d = pub_device()
    try:
        cov = d.coverage()
        recs, total = d.mul_batch(ks, cap=len(ks) + 16)
        live = [i for i, k in enumerate(ks) if k % orc.N]
        assert total == len(recs) == len(live) and all(int(r["compressed"]) == 5 and int(r["endo"]) == 0 for r in recs)
        assert sorted(int(r["key_offset"]) for r in recs) == live
        for r in recs:  # every scalar against the yardstick
            assert tuple(int(v) for v in r["h160"]) == h160_of(ks[int(r["key_offset"])]), int(r["key_offset"])
        now = d.coverage()
        assert tuple(b - a for a, b in zip(cov, now)) == (len(ks), len(ks), len(ks))
        phrases = [bytes(rnd.randrange(32, 127) for _ in range(1 + i % 70)) for i in range(3000)]
        recs, total = d.mul_batch_raw(phrases, cap=4096)
        sc = [int.from_bytes(hashlib.sha256(p).digest(), "big") for p in phrases]
        assert total == len(recs) == len(phrases)
        assert sorted((int(r["key_offset"]), tuple(int(v) for v in r["h160"])) for r in recs) == sorted((i, h160_of(k)) for i, k in enumerate(sc))
    finally:
        d.close()


def test_drop_round_fails_add_and_mul_and_the_next_call_is_clean():
    """one provoked COUNT mismatch each (only a loop bound shrinks): the call returns ECL_E_COVERAGE, the next one is whole"""
    from ecloop_amd import EclError
    d = pub_device(synth_bloom_words(4099, 3, "a|b"))
    try:
        d.set_geometry(8, 256)
        n, A = 1 << 17, 0x7_0000_0000
        good, _ = d.add_range(A, n)
        cov = d.coverage()
        d.diag_drop_round()
        with pytest.raises(EclError) as e:
            d.add_range(A, n)
        assert e.value.code == -8 and len(d.fetch_found(0, 16)) == 0
        now = d.coverage()
        assert now[0] - cov[0] == n and now[1] == cov[1] and now[2] - cov[2] < n
        recs, total = d.add_range(A, n)
        assert total == len(recs) and rec_set(recs) == rec_set(good) and len(recs) > 100
        after = d.coverage()
        assert after[0] - now[0] == after[1] - now[1] == after[2] - now[2] == n
        ks = [0xC0FFEE + 104729 * i for i in range(1000)]
        good, _ = d.mul_batch(ks)
        cov = d.coverage()
        d.diag_drop_round()
        with pytest.raises(EclError) as e:
            d.mul_batch(ks)
        assert e.value.code == -8
        now = d.coverage()
        assert now[0] - cov[0] == 1000 and now[1] == cov[1] and now[2] - cov[2] < 1000
        recs, total = d.mul_batch(ks)
        assert total == len(recs) and rec_set(recs) == rec_set(good)
        for r in recs:
            assert tuple(int(v) for v in r["h160"]) == h160_of(ks[int(r["key_offset"])])
    finally:
        d.close()


def test_lookahead_serves_pub_jobs_and_keeps_other_types_apart():
    """64 contiguous 2^21-key jobs on a pub context: calls are answered from sweeps and the records equal those of the same jobs with the
    look-ahead off; a `-a c` context on the same filter bits forms no group with it (its records stay its own)"""
    from ecloop_amd import Device
    words = synth_bloom_words(4099, 3, "a|b")  # passes one hash in ~300
    A, job, jobs = 0x300000000, 1 << 21, 64
    on, off = pub_device(words, lookahead=1 << 26), pub_device(words)
    c, cplain = Device(0), Device(0)
    try:
        for x, la in ((c, 1 << 26), (cplain, 0)):
            x.set_bloom(words)
            x.set_lookahead(la)
        cmine = []
        on.set_scan_end(A + jobs * job)
        mine, plain = [], []
        for j in range(jobs):
            recs, n = on.add_range(A + j * job, job, cap=1 << 15)
            assert n == len(recs)
            mine += rec_set(recs, A + j * job)
            if 20 <= j < 28:  # the other type walks the same jobs, inside what the pub sweeps hold
                crecs, cn = c.add_range(A + j * job, job, cap=1 << 15)
                assert cn == len(crecs)
                cmine += rec_set(crecs, A + j * job)
        crecs, cn = cplain.add_range(A + 20 * job, 8 * job, cap=1 << 18)
        assert cn == len(crecs) and sorted(cmine) == rec_set(crecs, A + 20 * job) and cmine and all(x[2] == 1 for x in cmine)
        for j in range(jobs):
            recs, n = off.add_range(A + j * job, job, cap=1 << 15)
            plain += rec_set(recs, A + j * job)
        sweeps, _, served, _ = on.lookahead_stats()
        assert sweeps >= 1 and served > 0, (sweeps, served)
        assert sorted(mine) == sorted(plain) and len(mine) > 100000 and all(x[2] == 5 for x in mine)
        for k, _, _, h in mine[:24]:
            assert h == h160_of(k)
        cov = on.coverage()
        assert cov[0] == cov[1] == jobs * job
    finally:
        on.close(), off.close(), c.close(), cplain.close()


def test_a_full_size_call_equals_its_parts():
    """one 2^30-key call against its four 2^28-key parts through a sparse filter (bit density 0.375: 3e-9 per key by chance) that holds
    keys at the ends of the call and of every part: the same records, every one re-derived by the yardstick, all planted keys present"""
    A, n, part = 0x9_0000_0000, 1 << 30, 1 << 28
    planted = sorted({0, 1, n - 1, n // 3} | {j * part + o for j in range(1, 4) for o in (-1, 0)} | {123456789, 987654321})
    d = pub_device(synth_bloom_words(1 << 16, 11, "a&(b|c)"))
    try:
        d.bloom_insert(np.array([list(h160_of(A + o)) for o in planted], np.uint32))
        before = d.coverage()
        whole, total = d.add_range(A, n, cap=1 << 16)
        assert total == len(whole)
        assert tuple(b - a for a, b in zip(before, d.coverage())) == (n, n, n)
        parts = []
        for j in range(4):
            recs, t = d.add_range(A + j * part, part, cap=1 << 16)
            assert t == len(recs)
            parts += rec_set(recs, j * part)
    finally:
        d.close()
    assert rec_set(whole) == sorted(parts)
    assert set(planted) <= {x[0] for x in parts} and len(parts) < 4096
    for off, endo, typ, h in parts:
        assert (endo, typ) == (0, 5) and h == h160_of(A + off), off


def test_cli_add_and_rnd_print_the_compressed_key_that_was_walked(cli, tmp_path):
    keys = (0xdc2a04, 0xffffff, 0x900001, 0x900002, 0x812345)
    assert {pub_ref.compressed(k)[:2] for k in keys} == {"02", "03"}  # both parities
    x = lambda k: "%064x" % orc.point_of(k)[0]
    unc = lambda k: "04%064x%064x" % orc.point_of(k)
    lst = tmp_path / "pub.txt"
    # the three forms; 0x900002 is listed as its NEGATIVE's compressed key (the other prefix byte): the key printed is the one walked
    lst.write_text("\n".join([pub_ref.compressed(keys[0]), x(keys[1]), unc(keys[2]), pub_ref.compressed(orc.N - keys[3]), pub_ref.compressed(keys[4])]) + "\n")
    want = sorted(pub_ref.found_line(k) for k in keys)
    r = run_cli(cli, ["add", "-f", str(lst), "-a", "x", "-r", "800000:ffffff"])
    assert r.found == want and counts(r.status) == (5, 8388608), (r.stdout, r.status)
    assert "~ endo: 0 ~ pub: 1 | filter: list (5)" in r.stdout
    blf = str(tmp_path / "pub.blf")
    subprocess.run([cli, "blf-gen", "-a", "x", "-n", "1000", "-o", blf], stdin=open(str(lst), "rb"), stdout=subprocess.PIPE, check=True, timeout=120)
    r = run_cli(cli, ["add", "-f", blf, "-a", "x", "-r", "800000:ffffff"])
    assert "filter: bloom" in r.stdout and r.found == want and counts(r.status) == (5, 8388608)
    # -endo: the list holds keys OUTSIDE the range whose images are inside: lambda k, -lambda^2 k; the key printed is the image's
    inside = (0x8abcde, 0xc00001, 0xfedcba)
    listed = [pub_ref.calc_priv(inside[0], 2), pub_ref.calc_priv(inside[1], 5), inside[2]]
    el = tmp_path / "endo.txt"
    el.write_text("".join(pub_ref.compressed(k) + "\n" for k in listed))
    r = run_cli(cli, ["add", "-f", str(el), "-a", "x", "-endo", "-r", "800000:ffffff"])
    # image 5 shares its x with image 4: the walked image is 4, whose key is the negative of the listed one
    assert r.found == sorted(pub_ref.found_line(k) for k in (listed[0], orc.N - listed[1], listed[2])), r.stdout
    assert counts(r.status) == (3, 6 * 8388608) and "~ endo: 1 ~ pub: 1 |" in r.stdout
    one = tmp_path / "dc.txt"
    one.write_text(pub_ref.compressed(0xdc2a04) + "\n")
    r = run_cli(cli, ["rnd", "-f", str(one), "-a", "x", "-seed", "pubkey", "-r", "800000:ffffff", "-d", "0:23"])
    assert r.found == [pub_ref.found_line(0xdc2a04)], r.stdout


def test_cli_mul_and_mul_raw_report_the_planted_keys(cli, tmp_path):
    lines = [l.strip() for l in open(os.path.join(GOLD, "mul_scalars.txt")) if l.strip()]
    picked = [orc.sn_from_hex(lines[i]) for i in (3, 77, 200)]
    phrases = [b"pubkey test phrase", b"correct horse battery staple", b"satoshi"]
    others = [b"phrase %d" % i for i in range(2000)]
    pks = [int.from_bytes(hashlib.sha256(p).digest(), "big") for p in phrases]
    lst = tmp_path / "planted.txt"
    lst.write_text("".join(pub_ref.compressed(k) + "\n" for k in picked + pks))
    r = run_cli(cli, ["mul", "-f", str(lst), "-a", "x"], stdin_path=os.path.join(GOLD, "mul_scalars.txt"))
    assert r.found == sorted(pub_ref.found_line(k) for k in picked), r.stdout
    assert "~ pub: 1 |" in r.stdout
    ph = tmp_path / "phrases.txt"
    ph.write_bytes(b"\n".join(others[:1000] + phrases + others[1000:]) + b"\n")
    r = run_cli(cli, ["mul", "-raw", "-f", str(lst), "-a", "x"], stdin_path=str(ph))
    assert r.found == sorted(pub_ref.found_line(k) for k in pks), r.stdout
