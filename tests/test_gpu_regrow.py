"""One context through calls that make its buffers grow, stay and grow again (csrc/devbuf.h: every device and page-locked buffer of a
context is a growable member that frees itself): the lane centres, the centre table, the chains and the table of `add` across two
geometries, filters of different sizes and a list that comes and goes; the staging, the parking space and the page-locked staging of `mul`
across a piece size; Taproot's slab and parking space; the herd of `kangaroo`; the record buffer under ecl_hip_fetch_found.

Every call is checked against what the suite trusts already - tests/mul_ref.py (the oracle's hashes and points of an array of scalars,
consecutive ones for `add`; Taproot through tests/tr_ref.py's formulas) and tests/kangaroo_ref.py: equal record sets, each record once,
and the three coverage totals grown by exactly the call's keys.  Every assertion is an equality.

The text and line buffers of `mul -raw` grow only past 16 MB of text or 2^20 lines: too large for this suite, that site is checked by
reading."""
import ctypes as C
import functools

import numpy as np
import pytest

import kangaroo_ref
import mul_ref
import orc
from mul_ref import FILTER3, ONES, START, canon, consecutive, difference
from synth import synth_bloom_words

pytestmark = pytest.mark.gpu

@functools.lru_cache(maxsize=None)
def random_ref(n):
    return mul_ref.MulRef(mul_ref.scalars()[0][:n])


def checked(d, what, call, want, nkeys):
    """one add / mul call: the records are the reference's, each once, the total their number, the coverage totals grow by the call's keys"""
    before = d.coverage()
    recs, total = call()
    grown = tuple(b - a for a, b in zip(before, d.coverage()))
    print("%s: %d records of %d expected, coverage +%s" % (what, total, len(want), grown))
    assert total == len(recs) == len(want), what
    assert difference(canon(recs), want) == "", what
    assert grown == (nkeys, nkeys, nkeys), what
    return recs


def test_add_across_geometries_filters_and_a_list():
    from ecloop_amd import Device
    small, large = 1 << 12, 1 << 15
    ref = consecutive(small + large + small)
    three = synth_bloom_words(*FILTER3)
    assert len(three) != len(ONES)
    want1 = ref.records("c", 0, small, FILTER3)
    bloom2 = ref.records("c", small, large, FILTER3)
    listed = sorted({tuple(int(w) for w in h) for h in bloom2["h160"][::2]})  # word by word: the order ecl_hip_set_list asks for
    in_list = np.array([tuple(int(w) for w in h) in set(listed) for h in bloom2["h160"]], bool)
    want2, want3 = bloom2[in_list], ref.records("c", small + large, small)
    assert 0 < len(want1) < small and 0 < len(want2) < len(bloom2) and len(want3) == small  # (the expectation)
    d = Device(0)
    try:
        d.set_bloom(ONES)
        d.set_bloom(three)  # a filter replaced by one of another size
        d.set_geometry(8, 256)
        checked(d, "2^12 keys at (8, 256), three-word filter", lambda: d.add_range(START, small, cap=small + 16), want1, small)
        d.set_geometry(16, 512)  # more lanes, longer chains, another table
        d.set_list(np.array(listed, np.uint32))  # ... and a record buffer of twice the size
        assert d.plan_geometry(large)[:2] == (16, 512)
        checked(d, "2^15 keys at (16, 512), list of %d" % len(listed), lambda: d.add_range(START + small, large, cap=large + 16), want2, large)
        d.set_list(None)
        d.set_bloom(ONES)
        d.set_geometry(8, 256)  # nothing grows: the table is rebuilt, the rest is large enough
        last = checked(d, "2^12 keys at (8, 256), all-ones filter", lambda: d.add_range(START + small + large, small, cap=small + 16), want3, small)
        # the records are still on the device, and stay there through a reserve that the record buffer is large enough for
        assert difference(canon(d.fetch_found(0, small)), want3) == "" and difference(canon(last), want3) == ""
        d.reserve(small, cap=small)
        assert difference(canon(d.fetch_found(0, small)), want3) == ""
        assert len(d.fetch_found(small - 5, 100)) == 5
    finally:
        d.close()


def test_mul_across_a_piece_size_pageable_and_page_locked():
    from ecloop_amd import Device, capi
    few, many = 1 << 10, (1 << 16) + 1  # the staging and the parking space of a piece: 2^16 scalars, then 2^17
    ref = random_ref(many)
    want_few, want_many = ref.records("c", 0, few), ref.records("c", 0, many)
    assert len(want_few) == int(ref.ok[:few].sum()) and len(want_many) == int(ref.ok.sum())
    K = np.ascontiguousarray(ref.K)

    def call(ptr, n):
        out = np.zeros(n + 16, dtype=capi.FOUND_DTYPE)
        cnt = C.c_uint32()
        assert d.lib.ecl_hip_mul_batch(d.h, ptr, n, out.ctypes.data, len(out), C.byref(cnt)) == 0
        return out[: cnt.value], cnt.value
    d = Device(0)
    ptr = d.lib.ecl_hip_alloc_host(K.nbytes)  # page-locked by the runtime and above 1 MB: read by DMA, no staging
    try:
        assert ptr and K.nbytes >= 1 << 20
        np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=K.shape)[:] = K
        d.set_bloom(ONES)
        checked(d, "2^10 scalars, staged", lambda: call(K.ctypes.data, few), want_few, few)
        checked(d, "2^16 + 1 scalars, page-locked", lambda: call(ptr, many), want_many, many)  # the device buffers grow, the staging does not
        checked(d, "2^10 scalars, staged again", lambda: call(K.ctypes.data, few), want_few, few)  # ... now it does
        checked(d, "2^16 + 1 scalars, pageable", lambda: call(K.ctypes.data, many), want_many, many)
        checked(d, "2^10 scalars, page-locked but small: staged", lambda: call(ptr, few), want_few, few)
    finally:
        d.close()
        if ptr:
            d.lib.ecl_hip_free_host(ptr)


def test_taproot_slab_and_parking_space_then_mul():
    from ecloop_amd import Device
    first, second = 1 << 10, 1 << 12
    ref = consecutive(first + second)
    d = Device(0, a33=False, tr=True)
    try:
        d.set_bloom(ONES)
        checked(d, "add, 2^10 keys", lambda: d.add_range(START, first, cap=first + 16), ref.records("t", 0, first), first)
        checked(d, "add, 2^12 keys", lambda: d.add_range(START + first, second, cap=second + 16), ref.records("t", first, second), second)
        checked(d, "mul, 2^10 scalars", lambda: d.mul_batch(mul_ref.ints_of(ref.K[:first]), cap=first + 16), ref.records("t", 0, first), first)
        checked(d, "add, 2^10 keys again", lambda: d.add_range(START, first, cap=first + 16), ref.records("t", 0, first), first)
    finally:
        d.close()


def test_herd_grows_and_shrinks():
    from ecloop_amd import Device
    key, base, dp, steps = 0x123456789, 0x100000000, 1, 6
    q = orc.point_of(key)

    def rec_set(recs):
        return sorted((int(r["key_offset"]), tuple(int(v) for v in r["h160"]), int(r["endo"]), int(r["compressed"])) for r in recs)
    d = Device(0, a33=False, pub=True, herd=True, ord_offs=dp)
    try:
        for hl, seed in ((4, 11), (6, 12), (4, 13)):
            want = sorted(kangaroo_ref.Herd(base, q, seed, hl, 20, 30).run(steps, dp))
            assert 0 < len(want) < steps << hl  # (the expectation)
            before = d.coverage()
            recs, total = d.add_range(None, steps << hl, cap=(steps << hl) + 16, herd=(base, q, seed, hl, 20, 30))
            grown = tuple(b - a for a, b in zip(before, d.coverage()))
            assert total == len(recs) == len(want) and rec_set(recs) == want and grown == (steps << hl,) * 3, hl
    finally:
        d.close()
