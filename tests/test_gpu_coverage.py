"""Key coverage on the GPU: every add_range / mul_batch / mul_batch_raw call compares the keys its kernels counted with the keys it asked for
(ECL_E_COVERAGE, include/ecloop_hip.h section 1).  Exact counts for every address-type set with and without -endo at awkward sizes and for
the headline's 2^32-key call; the test hook ecl_hip_diag_drop_round (one round short) turning into EclError(-8) for add, mul and mul -raw,
with the next calls whole again and equal to the oracle; a look-ahead sweep that miscounts is never used; the host program stopping on it,
and printing its coverage lines under ECLOOP_HIP_STATS."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import orc
from support import GOLD, cli, counts, rec_set, run_cli
from synth import synth_bloom_words

pytestmark = pytest.mark.gpu
G = json.load(open(os.path.join(GOLD, "golden.json")))["cases"]
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
SPARSE = synth_bloom_words(1 << 16, 5, "a|(b&c)")  # 0.625^20: a hit every ~12000 hashes
DENSER = synth_bloom_words(1 << 16, 8, "a|b")  # 0.75^20: a hit every ~300 hashes (`mul` calls of 1000 scalars have a few)
TYPES = {"c": dict(a33=True, a65=False, p2sh=False), "u": dict(a33=False, a65=True, p2sh=False), "cu": dict(a33=True, a65=True, p2sh=False),
         "s": dict(a33=False, a65=False, p2sh=True), "cs": dict(a33=True, a65=False, p2sh=True), "us": dict(a33=False, a65=True, p2sh=True),
         "cus": dict(a33=True, a65=True, p2sh=True)}
JOB = 1 << 21


def device(words, lookahead=0, **kw):
    from ecloop_amd import Device
    d = Device(0, **kw)
    d.set_lookahead(lookahead)
    d.set_bloom(words)
    return d


def add_lines(recs, start, stride=1):
    from ecloop_amd.capi import label_of
    from ecloop_amd.engine import calc_priv
    return sorted("%s\t%s\t%064x" % (label_of(r["compressed"]), orc.hex160(r["h160"]), calc_priv(start, stride, int(r["key_offset"]), int(r["endo"])))
                  for r in recs)


def oracle_add(words, start, nkeys, a33=True, a65=False, endo=False):  # (cmd_add's jobs: nkeys a multiple of 2048)
    rc, out, n, _, hashed = orc.add_range(orc.OrcFilter(bloom_words=words), start, start + nkeys, a33=a33, a65=a65, endo=endo, threads=4,
                                          cap=1 << 20)
    assert rc == 0 and hashed == nkeys
    return sorted(orc.found_lines(out, n))


def every_line(start, nkeys, a33, a65, endo):
    """the found lines of an all-ones filter: every key x image x selected type, hashed by the oracle"""
    from ecloop_amd.engine import calc_priv
    keys = [calc_priv(start, 1, off, e) for off in range(nkeys) for e in range(6 if endo else 1)]
    h33, h65, ok = orc.mul_hash160_many(np.array([[(k >> (64 * i)) & orc.MASK64 for i in range(4)] for k in keys], np.uint64), a33=True, a65=True)
    assert ok.all()
    return sorted([("addr33\t%s\t%064x" % (orc.hex160(h33[j]), k)) for j, k in enumerate(keys) if a33] +
                  [("addr65\t%s\t%064x" % (orc.hex160(h65[j]), k)) for j, k in enumerate(keys) if a65])


def grows(d, before, by):
    now = d.coverage()
    assert tuple(b - a for a, b in zip(before, now)) == (by, by, by), (before, now, by)
    return now


@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
@pytest.mark.parametrize("types", list(TYPES))
def test_add_counts_every_key_of_every_call(types, endo):
    """look-ahead off: each call returns OK and all three totals grow by exactly its keys; on the all-ones filter every key x type x image
    is reported once, and for the sets the oracle knows (c, u, cu) the records are the oracle's"""
    t = TYPES[types]
    per_key = sum(t.values()) * (6 if endo else 1)
    d = device(ONES, endo=endo, **t)
    try:
        cov = d.coverage()
        start = 0x1234567
        for n in (1, 2047, 2049):
            recs, total = d.add_range(start, n, cap=n * per_key + 16)
            assert total == len(recs) == n * per_key
            cov = grows(d, cov, n)
            if not t["p2sh"]:
                assert add_lines(recs, start) == every_line(start, n, t["a33"], t["a65"], endo), (types, n)
            start += n
        d.set_bloom(SPARSE)
        cov = d.coverage()
        for n in ((1 << 21) + 777, 1 << 24):
            _, total = d.add_range(start, n, cap=4096)
            cov = grows(d, cov, n)
            start += n
        assert cov[0] == cov[1] <= cov[2]
    finally:
        d.close()


def test_add_headline_call_of_2_32_keys():
    d = device(SPARSE)
    try:
        cov = d.coverage()
        d.add_range(0x4000_0000_0000, 1 << 32, cap=4096)
        grows(d, cov, 1 << 32)
    finally:
        d.close()


@pytest.mark.parametrize("types", ["c", "u", "cu", "cs"])
def test_mul_counts_every_scalar(types):
    """mul_batch at 1, 1000 and 2^20 + 3 scalars (two of them = 0 (mod n): nothing to hash, counted all the same) and mul_batch_raw at
    2^16 + 5 lines: covered grows by n; records of the 1000-scalar call equal the oracle's where it knows the types"""
    t = TYPES[types]
    d = device(DENSER, **t)
    try:
        cov = d.coverage()
        for n in (1, 1000, (1 << 20) + 3):
            ks = [0x51_7e57_0000 + 7919 * i for i in range(n)]
            if n > 2:
                ks[1], ks[n // 2] = 0, orc.N
            recs, total = d.mul_batch(ks, cap=1 << 16)
            cov = grows(d, cov, n)
            if n == 1000 and not t["p2sh"]:  # (the oracle's batch has no point at infinity: it is given the other scalars)
                rc, out, no = orc.mul_batch(orc.OrcFilter(bloom_words=DENSER), [k for k in ks if k % orc.N], a33=t["a33"], a65=t["a65"])
                assert rc == 0 and total == no == len(recs)
                assert sorted((orc.hex160(r["h160"]), ks[int(r["key_offset"])]) for r in recs) == \
                    sorted((orc.hex160(out[i].h160), orc.val(out[i].pk)) for i in range(no))
        lines = [b"cover %d" % i for i in range((1 << 16) + 5)]
        d.mul_batch_raw(lines, cap=1 << 16)
        grows(d, cov, len(lines))
    finally:
        d.close()


def test_drop_round_fails_an_add_call_and_the_walk_is_repositioned():
    """a call whose launch ran one group per lane short returns -8 with nothing to fetch and device < requested; the same range again and the
    next contiguous call are whole and equal to the oracle (the walk state left by the short launch was dropped)"""
    from ecloop_amd import EclError
    n = 1 << 17
    d = device(SPARSE)
    try:
        d.set_geometry(8, 256)  # 32 groups per lane: the short launch leaves its centres 31 groups on, where no call expects them
        B, T, nb = d.plan_geometry(n)
        assert T * 2 * B * nb == n and nb >= 2  # an exact launch: a whole call would leave its walk ready for the next contiguous one
        A = 0x7_0000_0000
        recs, _ = d.add_range(A, n)
        assert add_lines(recs, A) == oracle_add(SPARSE, A, n)
        cov = d.coverage()
        d.diag_drop_round()
        with pytest.raises(EclError) as e:
            d.add_range(A + n, n)
        assert e.value.code == -8 and "every key" in str(e.value)
        assert len(d.fetch_found(0, 16)) == 0
        now = d.coverage()
        assert now[0] - cov[0] == n and now[1] == cov[1] and now[2] - cov[2] < n
        requested, covered, dev = now
        assert dev < requested and covered < requested
        for start in (A + n, A + 2 * n):
            recs, total = d.add_range(start, n)
            assert total == len(recs) and add_lines(recs, start) == oracle_add(SPARSE, start, n), hex(start)
        after = d.coverage()
        assert after[0] - now[0] == after[1] - now[1] == after[2] - now[2] == 2 * n
    finally:
        d.close()


def test_drop_round_fails_mul_and_mul_raw():
    from ecloop_amd import EclError
    d = device(DENSER, a33=True, a65=True)
    try:
        ks = [0xC0FFEE + 104729 * i for i in range(1000)]
        rc, out, no = orc.mul_batch(orc.OrcFilter(bloom_words=DENSER), ks, a33=True, a65=True)
        want = sorted((orc.hex160(out[i].h160), orc.val(out[i].pk)) for i in range(no))
        cov = d.coverage()
        d.diag_drop_round()
        with pytest.raises(EclError) as e:
            d.mul_batch(ks)
        assert e.value.code == -8
        now = d.coverage()
        assert now[0] - cov[0] == 1000 and now[1] == cov[1] and now[2] - cov[2] < 1000
        recs, total = d.mul_batch(ks)
        assert total == len(recs) and sorted((orc.hex160(r["h160"]), ks[int(r["key_offset"])]) for r in recs) == want
        lines = [b"phrase %d" % i for i in range((1 << 16) + 5)]
        good, ngood = d.mul_batch_raw(lines, cap=1 << 16)
        cov = d.coverage()
        d.diag_drop_round()
        with pytest.raises(EclError) as e:
            d.mul_batch_raw(lines, cap=1 << 16)
        assert e.value.code == -8
        now = d.coverage()
        assert now[0] - cov[0] == len(lines) and now[1] == cov[1] and now[2] - cov[2] < len(lines)
        recs, total = d.mul_batch_raw(lines, cap=1 << 16)
        assert total == ngood and rec_set(recs) == rec_set(good)
        # the raw records against the oracle on the SHA-256 scalars of their lines
        sc = [int.from_bytes(hashlib.sha256(l).digest(), "big") for l in lines]
        rc, out, no = orc.mul_batch(orc.OrcFilter(bloom_words=DENSER), sc, a33=True, a65=True)
        assert rc == 0 and no == total
        assert sorted((orc.hex160(r["h160"]), sc[int(r["key_offset"])] % orc.N) for r in recs) == \
            sorted((orc.hex160(out[i].h160), orc.val(out[i].pk)) for i in range(no))
    finally:
        d.close()


def test_lookahead_never_publishes_a_sweep_that_miscounts():
    """contiguous 2^21-key jobs with the look-ahead on: served calls are covered (requested == covered, device >= covered); the job whose
    sweep runs short returns -8, no later job is served from a sweep, and every later job has the records of a look-ahead-off run"""
    from ecloop_amd import EclError
    A, jobs = 0x2_0000_0000, 24
    p, a = device(SPARSE), device(SPARSE, lookahead=1 << 24)
    try:
        a.set_scan_end(A + jobs * JOB)
        for j in range(9):  # job 0 launches, job 1 sweeps jobs 1 ... 8 (2^24 keys), 2 ... 8 are served from that sweep
            want, nw = p.add_range(A + j * JOB, JOB)
            got, ng = a.add_range(A + j * JOB, JOB)
            assert ng == nw and rec_set(got) == rec_set(want), j
        sweeps, swept, served, _ = a.lookahead_stats()
        req, cov, dev = a.coverage()
        assert sweeps == 1 and served == 8 and req == cov == 9 * JOB and dev >= cov
        a.diag_drop_round()  # job 9 finds nothing prepared and starts the next sweep: that sweep runs short
        with pytest.raises(EclError) as e:
            a.add_range(A + 9 * JOB, JOB)
        assert e.value.code == -8
        assert a.lookahead_stats()[:3] == (sweeps, swept, served)
        for j in range(9, jobs):  # job 9 again, then the rest: launched, none served
            want, nw = p.add_range(A + j * JOB, JOB)
            got, ng = a.add_range(A + j * JOB, JOB)
            assert ng == nw and rec_set(got) == rec_set(want), j
        assert a.lookahead_stats()[2] == served
        req2, cov2, dev2 = a.coverage()
        assert req2 - req == (jobs - 8) * JOB and cov2 - cov == (jobs - 9) * JOB and dev2 >= cov2
    finally:
        p.close(), a.close()


def digest(lines):
    return hashlib.sha256(("\n".join(lines) + "\n").encode()).hexdigest()


CASES = {"add": (["add", "-f", os.path.join(GOLD, "btc-puzzles-hash"), "-r", "8000:ffffff"], None, "make_add_8000_ffffff"),
         "mul": (["mul", "-f", os.path.join(GOLD, "btc-bw-hash"), "-a", "cu"], os.path.join(GOLD, "btc-bw-priv"), "make_mul_bw")}


@pytest.mark.parametrize("case", list(CASES))
def test_cli_stops_on_a_miscount_and_reports_coverage(cli, tmp_path, case):
    args, stdin_path, gold = CASES[case]
    g = G[gold]
    # the hook (armed on every context: `mul` hands its one batch to either of its two): exit status 1, the library's text on stderr,
    # no found line written
    r = run_cli(cli, args, out=str(tmp_path / "drop.txt"), stdin_path=stdin_path, env={"ECLOOP_HIP_TEST_DROP_ROUND": "1"}, check=False)
    assert r.returncode == 1 and "[!] " in r.stderr and "did not hash every key" in r.stderr, r.stderr[-500:]
    assert r.lines == []
    # without it: the found lines and status counters of the golden run, and no coverage line unless asked for
    r = run_cli(cli, args, out=str(tmp_path / "plain.txt"), stdin_path=stdin_path, check=False)
    assert r.returncode == 0 and len(r.lines) == g["count"] and digest(r.lines) == g["sha256_sorted"] and counts(r.status) == (g["status_found"], g["status_checked"])
    assert "coverage" not in r.stdout + r.stderr
    r = run_cli(cli, args, out=str(tmp_path / "stats.txt"), stdin_path=stdin_path, env={"ECLOOP_HIP_STATS": "1"}, check=False)
    out, err = r.stdout, r.stderr
    assert r.returncode == 0 and digest(r.lines) == g["sha256_sorted"]  # (the stats lines follow the status line on stderr)
    pat = r"^gpu (\d+) coverage: requested (\d+), covered (\d+), device (\d+)$" if case == "add" else \
        r"^mul context (\d+) coverage: requested (\d+), covered (\d+), device (\d+)$"
    found = re.findall(pat, out if case == "add" else err, re.M)
    assert found and all(int(r) == int(c) <= int(dv) for _, r, c, dv in found), found
    total = sum(int(r) for _, r, _, _ in found)
    assert total == (g["status_checked"] if case == "add" else 1080)
    if case == "add":  # one line per context, beside (and not matching) the existing per-context line
        assert len(found) == len(re.findall(r"^gpu \d+: (\d+) launches", out, re.M))
