"""The state a search call leaves behind, for each of the library's five call bodies (add, add on a Taproot context, the herd, mul,
mul -raw): the result code, the total, the records delivered and those ecl_hip_fetch_found still brings, and what the call booked - the
three coverage totals, launches and keys, set-ups, mul calls and scalars.  Whole calls, calls past the caller's cap (with and without a
list), contiguous and re-positioned ones, and calls the test hook ecl_hip_diag_drop_round makes fall short: those end in
ECL_E_COVERAGE with nothing to fetch, are booked as launched, and drop the resident walk or herd.

Record sets are the reference's (tests/mul_ref.py over consecutive scalars, tests/kangaroo_ref.py); every assertion is an equality,
but for the device count of a short call, which is only known to be smaller than the keys asked for."""
import hashlib

import numpy as np
import pytest

import kangaroo_ref
import mul_ref
import orc
from mul_ref import ONES, START, canon, consecutive, difference

pytestmark = pytest.mark.gpu
N = 8192          # keys of an `add` call: at (8, 256) every lane walks two groups, and the launch is exact
REF = 5 * N       # the consecutive scalars all `add` cases share


def snap(d):
    return d.coverage(), d.timing()[1:], d.setup_timing()[1], d.mul_timing()[1:]


def booked(d, call):
    """-> (what call() returns, or the EclError it raises; coverage deltas; (launches, keys) deltas; set-ups delta; (mul calls, scalars) deltas)"""
    from ecloop_amd import EclError
    cov, tim, ups, mul = snap(d)
    try:
        res = call()
    except EclError as e:
        res = e
    cov2, tim2, ups2, mul2 = snap(d)
    sub = lambda a, b: tuple(y - x for x, y in zip(a, b))
    out = res, sub(cov, cov2), sub(tim, tim2), ups2 - ups, sub(mul, mul2)
    print("total %s, booked %s" % (res if isinstance(res, EclError) else res[1], out[1:]))
    return out


def same(recs, want):
    return difference(canon(recs), want)


def short_call(d, call, what, n, launches=1, is_mul=False):
    """a call after diag_drop_round: E_COVERAGE naming the call, booked as launched, nothing to fetch -> the set-ups it booked"""
    from ecloop_amd import capi
    d.diag_drop_round()
    res, cov, tim, ups, mul = booked(d, call)
    assert isinstance(res, capi.EclError) and res.code == capi.E_COVERAGE
    assert cov[:2] == (n, 0) and 0 <= cov[2] < n
    assert str(res).endswith("%s: the device hashed %d keys of the %d asked for" % (what, cov[2], n))
    assert (tim, mul) == (((0, 0), (1, n)) if is_mul else ((launches, n), (0, 0)))
    assert len(d.fetch_found(0, 16)) == 0
    return ups


def test_add_whole_past_the_cap_listed_and_short():
    from ecloop_amd import Device
    ref = consecutive(REF)
    part = [ref.records("c", i * N, N) for i in range(3)]
    assert all(len(p) == N for p in part)  # (the expectation: every key once)
    hashes = [tuple(int(w) for w in h) for h in part[1]["h160"]]
    listed = sorted(set(hashes[::2]))  # word by word: the order ecl_hip_set_list asks for
    in_list = np.array([h in set(listed) for h in hashes], bool)
    assert 100 < in_list.sum() < N
    d = Device(0)
    try:
        d.set_bloom(ONES)
        d.set_geometry(8, 256)
        assert d.plan_geometry(N) == (8, 256, 2)
        (recs, total), cov, tim, ups, mul = booked(d, lambda: d.add_range(START, N, cap=N + 16))
        assert total == len(recs) == N and same(recs, part[0]) == ""
        assert (cov, tim, ups, mul) == ((N, N, N), (1, N), 1, (0, 0))
        # the contiguous next call, past the caller's cap: the first 100 delivered, the rest still on the device
        (recs, total), cov, tim, ups, mul = booked(d, lambda: d.add_range(START + N, N, cap=100))
        rest = d.fetch_found(100, N)
        assert total == N and len(recs) == 100 and len(rest) == N - 100 and same(np.concatenate([recs, rest]), part[1]) == ""
        assert (cov, tim, ups, mul) == ((N, N, N), (1, N), 0, (0, 0))
        # a call that does not continue the walk
        (recs, total), cov, tim, ups, mul = booked(d, lambda: d.add_range(START, N, cap=N + 16))
        assert total == len(recs) == N and same(recs, part[0]) == ""
        assert (cov, tim, ups, mul) == ((N, N, N), (1, N), 1, (0, 0))
        # a list of every second hash, and a cap below the confirmed count: the total is the confirmed count, the rest comes from the confirmed half
        d.set_list(np.array(listed, np.uint32))
        (recs, total), cov, tim, ups, mul = booked(d, lambda: d.add_range(START + N, N, cap=100))
        rest = d.fetch_found(100, N)
        assert total == in_list.sum() and len(recs) == 100 and len(rest) == total - 100
        assert same(np.concatenate([recs, rest]), part[1][in_list]) == ""
        assert (cov, tim, ups, mul) == ((N, N, N), (1, N), 0, (0, 0))
        d.set_list(None)
        # one round short: the contiguous call fails, and the same call again re-positions
        call = lambda: d.add_range(START + 2 * N, N, cap=N + 16)
        assert short_call(d, call, "add_range", N) == 0
        (recs, total), cov, tim, ups, mul = booked(d, call)
        assert total == len(recs) == N and same(recs, part[2]) == ""
        assert (cov, tim, ups, mul) == ((N, N, N), (1, N), 1, (0, 0))
    finally:
        d.close()


def test_add_from_an_origin():
    from ecloop_amd import Device
    ref = consecutive(REF)
    d = Device(0, a33=False, pub=True, origin=True)
    try:
        d.set_bloom(ONES)
        d.set_geometry(8, 256)
        # O = m G: the call walks the keys START + m + j
        (recs, total), cov, tim, ups, mul = booked(d, lambda: d.add_range(START, N, cap=N + 16, origin=orc.point_of(N)))
        assert total == len(recs) == N and same(recs, ref.records("x", N, N)) == ""
        assert (cov, tim, ups, mul) == ((N, N, N), (1, N), 1, (0, 0))
        # the contiguous scalar from another origin: re-positioned
        (recs, total), cov, tim, ups, mul = booked(d, lambda: d.add_range(START + N, N, cap=N + 16, origin=orc.point_of(2 * N)))
        assert total == len(recs) == N and same(recs, ref.records("x", 3 * N, N)) == ""
        assert (cov, tim, ups, mul) == ((N, N, N), (1, N), 1, (0, 0))
    finally:
        d.close()


def mul_scalars(n):
    K = mul_ref.random_scalars(np.random.default_rng(17), n).copy()
    K[7], K[n - 100] = 0, np.array(mul_ref.limbs(orc.N), np.uint64)  # counted, not probed
    return mul_ref.MulRef(K)


def test_mul_whole_past_the_cap_and_short():
    from ecloop_amd import Device
    n = 300
    ref = mul_scalars(n)
    want, ks = ref.records("c"), mul_ref.ints_of(ref.K)
    assert len(want) == n - 2
    d = Device(0)
    try:
        d.set_bloom(ONES)
        (recs, total), cov, tim, ups, mul = booked(d, lambda: d.mul_batch(ks, cap=n + 16))
        assert total == len(recs) == n - 2 and same(recs, want) == ""
        assert (cov, tim, ups, mul) == ((n, n, n), (0, 0), 0, (1, n))
        (recs, total), cov, tim, ups, mul = booked(d, lambda: d.mul_batch(ks, cap=10))
        rest = d.fetch_found(10, n)
        assert total == n - 2 and len(recs) == 10 and len(rest) == n - 12 and same(np.concatenate([recs, rest]), want) == ""
        assert (cov, tim, ups, mul) == ((n, n, n), (0, 0), 0, (1, n))
        assert short_call(d, lambda: d.mul_batch(ks, cap=n + 16), "mul_batch", n, is_mul=True) == 0
    finally:
        d.close()


def test_mul_raw_whole_and_short():
    from ecloop_amd import Device
    n = 300
    lines = [b"phrase %d" % i for i in range(n)]
    K = np.array([np.frombuffer(hashlib.sha256(l).digest(), dtype=">u8")[::-1] for l in lines], np.uint64)
    want = mul_ref.MulRef(K).records("c")
    assert len(want) == n
    d = Device(0)
    try:
        d.set_bloom(ONES)
        (recs, total), cov, tim, ups, mul = booked(d, lambda: d.mul_batch_raw(lines, cap=n + 16))
        assert total == len(recs) == n and same(recs, want) == ""
        assert (cov, tim, ups, mul) == ((n, n, n), (0, 0), 0, (1, n))
        assert short_call(d, lambda: d.mul_batch_raw(lines, cap=n + 16), "mul_batch_raw", n, is_mul=True) == 0
    finally:
        d.close()


def test_taproot_add_in_four_slabs(monkeypatch):
    from ecloop_amd import Device
    monkeypatch.setenv("ECL_HIP_TR_SLAB_LOG2", "12")
    slab = 1 << 12
    n = 3 * slab + 77  # four slabs, the last one odd
    ref = consecutive(REF)
    d = Device(0, a33=False, tr=True)
    try:
        d.set_bloom(ONES)
        d.set_geometry(8, 256)  # a slab is one exact launch: it hands the walk to the next
        (recs, total), cov, tim, ups, mul = booked(d, lambda: d.add_range(START, n, cap=n + 16))
        assert total == len(recs) == n and same(recs, ref.records("t", 0, n)) == ""
        assert (cov, tim, ups, mul) == ((n, n, n), (4, n), 1, (0, 0))
        # the contiguous next call: the odd slab left no walk to continue
        (recs, total), cov, tim, ups, mul = booked(d, lambda: d.add_range(START + n, slab, cap=slab + 16))
        assert total == len(recs) == slab and same(recs, ref.records("t", n, slab)) == ""
        assert (cov, tim, ups, mul) == ((slab, slab, slab), (1, slab), 1, (0, 0))
        # ... and the one after a whole slab does
        (recs, total), cov, tim, ups, mul = booked(d, lambda: d.add_range(START + n + slab, slab, cap=slab + 16))
        assert total == len(recs) == slab and same(recs, ref.records("t", n + slab, slab)) == ""
        assert (cov, tim, ups, mul) == ((slab, slab, slab), (1, slab), 0, (0, 0))
        call = lambda: d.add_range(START + n + 2 * slab, n, cap=n + 16)
        assert short_call(d, call, "add_range (Taproot, points emitted)", n, launches=4) == 0
        (recs, total), cov, tim, ups, mul = booked(d, call)
        assert total == len(recs) == n and same(recs, ref.records("t", n + 2 * slab, n)) == ""
        assert (cov, tim, ups, mul) == ((n, n, n), (4, n), 1, (0, 0))
    finally:
        d.close()


def test_herd_whole_continued_rebuilt_and_short():
    from ecloop_amd import Device
    key, base, dp, steps, hl = 0x123456789, 0x100000000, 1, 6, 4
    q, n = orc.point_of(key), 6 << 4

    def rec_set(recs):
        return sorted((int(r["key_offset"]), tuple(int(v) for v in r["h160"]), int(r["endo"]), int(r["compressed"])) for r in recs)

    def walk(herd):
        return sorted(herd.run(steps, dp))
    one, two = kangaroo_ref.Herd(base, q, 11, hl, 20, 30), kangaroo_ref.Herd(base, q, 13, hl, 20, 30)
    d = Device(0, a33=False, pub=True, herd=True, ord_offs=dp)
    try:
        call = lambda seed: d.add_range(None, n, cap=n + 16, herd=(base, q, seed, hl, 20, 30))
        for seed, herd, set_ups in ((11, one, 1), (11, one, 0), (13, two, 1)):  # built, continued, another seed: built
            want = walk(herd)
            assert 0 < len(want) < n  # (the expectation)
            (recs, total), cov, tim, ups, mul = booked(d, lambda: call(seed))
            assert total == len(recs) == len(want) and rec_set(recs) == want
            assert (cov, tim, ups, mul) == ((n, n, n), (1, n), set_ups, (0, 0))
        assert short_call(d, lambda: call(13), "add_range", n) == 0
        want = walk(kangaroo_ref.Herd(base, q, 13, hl, 20, 30))  # the herd was dropped: from its start
        (recs, total), cov, tim, ups, mul = booked(d, lambda: call(13))
        assert total == len(recs) == len(want) and rec_set(recs) == want
        assert (cov, tim, ups, mul) == ((n, n, n), (1, n), 1, (0, 0))
    finally:
        d.close()
