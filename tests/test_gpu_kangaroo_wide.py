"""`kangaroo` on the GPU where the command is meant to run: distances above 2^64 and 2^96, distinguished points decided by limb 1 of x,
calls of more than one launch, a herd of two set-up chunks, the two refusals of the herd (a start at infinity, a distance past 2^128), zero
offsets, and a base above 2^128.  The inputs are constructed in tests/kangaroo_cases.py, which tests/test_kangaroo_cases.py checks without
a GPU; every assertion here is an equality with the yardstick (tests/kangaroo_ref.py over the oracle's points)."""
import numpy as np
import pytest

import kangaroo_cases as kc
import kangaroo_ref as ref
import orc

pytestmark = pytest.mark.gpu


def herd_device(dp):
    from ecloop_amd import Device
    return Device(0, a33=False, pub=True, herd=True, ord_offs=dp)


def rec_set(recs):
    return sorted((int(r["key_offset"]), tuple(int(v) for v in r["h160"]), int(r["endo"]), int(r["compressed"])) for r in recs)


def grown(before, after):
    return tuple(b - a for a, b in zip(before, after))


@pytest.mark.parametrize("name", list(kc.WIDE))
def test_wide_distances_bit_for_bit(name):
    """jb = 90, sb = 100 (and jb = sb = 64 at dp = 0) at a base of 2^200: all four words of the distance, the carry from word 1 into word 2,
    the table's high words and the record's swapped pair are in use (test_kangaroo_cases.py counts them); the sorted records of a call equal
    the yardstick's exactly, and the coverage totals grow by exactly the jumps"""
    hl, _, _, _, dp, steps = kc.WIDE[name]
    want, _ = kc.wide_run(name)
    d = herd_device(dp)
    try:
        before = d.coverage()
        recs, n = d.add_range(None, steps << hl, cap=len(want) + 64, herd=kc.wide_block(name))
        after = d.coverage()
    finally:
        d.close()
    assert n == len(recs) == len(want) and rec_set(recs) == list(want)
    assert all(int(r["compressed"]) == 6 for r in recs) and grown(before, after) == (steps << hl,) * 3


@pytest.mark.parametrize("name,dp,expected", [(name, dp, e) for name, t in kc.DP_TARGETS.items() for dp, e in t[2]],
                         ids=["%s-dp%d" % (name, dp) for name, t in kc.DP_TARGETS.items() for dp, _ in t[2]])
def test_dp_across_the_limb_boundary(name, dp, expected):
    """the first jump of wild kangaroo 1 lands on a point whose x has the low bits of the name (zero below bit 32, 31, 29 or 28, that bit
    set): a context opened with this dp reports that one record in 8 steps, or none, as the yardstick does"""
    want = kc.dp_run(name, dp)
    assert len(want) == (1 if expected else 0)
    d = herd_device(dp)
    try:
        before = d.coverage()
        recs, n = d.add_range(None, kc.DP_STEPS << kc.DP_HERD[1], cap=64, herd=kc.dp_target(name)[0])
        after = d.coverage()
    finally:
        d.close()
    assert n == len(recs) == len(want) and rec_set(recs) == list(want)
    assert grown(before, after) == (kc.DP_STEPS << kc.DP_HERD[1],) * 3


@pytest.mark.parametrize("name", list(kc.LONG))
def test_a_call_of_more_than_one_launch(name):
    """4096 + 4096 + 7 steps on two kangaroos, 4096 + 1 on a full lane: the launches of one call continue one another, and the call's records
    and jumps are the sum of theirs"""
    hl, _, _, _, dp, steps = kc.LONG[name]
    want = kc.long_run(name)
    d = herd_device(dp)
    try:
        d.reset_timing()
        before = d.coverage()
        recs, n = d.add_range(None, steps << hl, cap=len(want) + 64, herd=kc.long_block(name))
        after, setups = d.coverage(), d.setup_timing()[1]
    finally:
        d.close()
    assert n == len(recs) == len(want) and rec_set(recs) == list(want)
    assert grown(before, after) == (steps << hl,) * 3 and setups == 1


def test_two_long_calls_continue_one_another():
    """the 8199 steps of H2 as a call of 4097 and a contiguous one of 4102, each of two launches: one set-up, the records of the single call,
    the coverage whole each time"""
    hl, _, _, _, dp, steps = kc.LONG["H2"]
    want = kc.long_run("H2")
    d = herd_device(dp)
    try:
        d.reset_timing()
        parts, cov = [], [d.coverage()]
        for s in kc.LONG_SPLIT:
            recs, n = d.add_range(None, s << hl, cap=len(want) + 64, herd=kc.long_block("H2"))
            assert n == len(recs)
            parts.append(recs)
            cov.append(d.coverage())
        setups = d.setup_timing()[1]
    finally:
        d.close()
    assert setups == 1 and rec_set(np.concatenate(parts)) == list(want)
    assert [grown(a, b) for a, b in zip(cov, cov[1:])] == [(s << hl,) * 3 for s in kc.LONG_SPLIT]


def test_a_herd_of_two_setup_chunks():
    """2^19 kangaroos, dp = 0, one step: every kangaroo's first jump is a record.  A record does not name its kangaroo, so (1) over all
    records: the distance less exactly one s_j is an offset r_i of the record's herd, and the offsets so matched are all of that herd's, each
    once; (2) for 64 kangaroos - the ends of both set-up chunks and 54 seeded ones - the whole expected record (start by the oracle, one
    jump by the yardstick's rule) is among the results"""
    hl = kc.BIG[0]
    H = 1 << hl
    s, r = kc.big_herd()
    d = herd_device(0)
    try:
        d.reset_timing()
        before = d.coverage()
        recs, n = d.add_range(None, H, cap=H + 64, herd=kc.big_block())
        after, setups = d.coverage(), d.setup_timing()[1]
    finally:
        d.close()
    assert n == len(recs) == H and setups == 1 and grown(before, after) == (H,) * 3
    assert (recs["compressed"] == 6).all() and not recs["h160"][:, :2].any() and int(recs["key_offset"].max()) < 1 << 63
    S = np.array(s, np.uint64)
    for par in (0, 1):
        R = np.sort(np.array(r[par::2], np.uint64))
        dist = recs["key_offset"][recs["endo"] == par]
        assert len(dist) == H // 2
        hits, matched = np.zeros(len(dist), np.int64), np.zeros(len(dist), np.uint64)
        for sj in S:
            ok = dist >= sj
            cand = np.where(ok, dist - sj, 0).astype(np.uint64)
            at = np.minimum(np.searchsorted(R, cand), len(R) - 1)
            hit = ok & (R[at] == cand)
            hits += hit
            matched[hit] = cand[hit]
        assert (hits == 1).all() and np.array_equal(np.sort(matched), R), par
    key = recs["key_offset"]
    for i, want in kc.big_expected().items():
        got = rec_set(recs[key == np.uint64(want[0])])
        assert got == [want], (i, got, want)


def infinity_then_good(blk):
    """a block with a start at infinity on a fresh context -> (error code, the totals across the refused call, set-ups of it, the records
    and the total of the good block behind it, the totals across that, set-ups of that)"""
    from ecloop_amd import capi
    with pytest.raises(ValueError):
        ref.Herd(*blk)
    hl = kc.ODD[1]
    d = herd_device(3)
    try:
        d.reset_timing()
        c0 = d.coverage()
        with pytest.raises(capi.EclError) as e:
            d.add_range(None, kc.ODD_GOOD_STEPS << hl, cap=4096, herd=blk)
        c1, s1 = d.coverage(), d.setup_timing()[1]
        recs, n = d.add_range(None, kc.ODD_GOOD_STEPS << hl, cap=4096, herd=kc.odd_good_block())
        c2, s2 = d.coverage(), d.setup_timing()[1]
    finally:
        d.close()
    return e.value.code, grown(c0, c1), s1, rec_set(recs), n, grown(c1, c2), s2 - s1


@pytest.mark.parametrize("which", ["wild", "tame"])
def test_a_start_at_infinity_is_refused(which):
    """Q = (n - r_1) G puts wild kangaroo 1, base = n - r_0 tame kangaroo 0 on the point at infinity: E_RANGE where the yardstick raises
    ValueError.  The call is refused before any jump: none of the three coverage totals moves and no set-up is booked (the call leaves in
    the middle of its frame: rc_was_launched of callstate.h is false for it, as documented).  A good block on the same context then gives
    the yardstick's records with one set-up and whole coverage"""
    from ecloop_amd import capi
    blk = kc.wild_infinity_block() if which == "wild" else kc.tame_infinity_block()
    code, across, setups, recs, n, after, setups_good = infinity_then_good(blk)
    jumps = kc.ODD_GOOD_STEPS << kc.ODD[1]
    assert code == capi.E_RANGE and across == (0, 0, 0) and setups == 0
    assert n == len(recs) and recs == list(kc.odd_good_run()) and after == (jumps,) * 3 and setups_good == 1


def test_zero_offsets():
    """sb = 1: every offset is 0 or 1.  A wild kangaroo with r_i = 0 starts on Q itself (k_herd_init's branch for a product that is the point
    at infinity), a tame one on base G; kangaroos with equal offsets walk together in one lane.  The records of 64 steps at dp = 0,
    duplicates included, are the yardstick's"""
    _, hl, _, _, dp, steps = kc.ZERO
    want = kc.zero_run()
    d = herd_device(dp)
    try:
        before = d.coverage()
        recs, n = d.add_range(None, steps << hl, cap=len(want) + 64, herd=kc.zero_block())
        after = d.coverage()
    finally:
        d.close()
    assert n == len(recs) == len(want) == steps << hl and rec_set(recs) == list(want) and grown(before, after) == (steps << hl,) * 3


def test_a_distance_past_2_128_is_refused():
    """jb = 120, sb = 124 on two kangaroos: the yardstick raises OverflowError in step k.  k - 1 steps are the yardstick's records, all four
    words of the distance in use; one more contiguous step is E_RANGE; a call of k steps (the herd built anew: the refusal dropped it) is
    E_RANGE; the block again with k - 1 steps builds the herd anew and gives the same records.
    Coverage across a call refused for its distance, pinned to what the library does: the launches ran and the device counted their jumps, so
    the `device` total grows by them, while `requested` and `covered` stay (the call is booked as refused; its set-up, if it had one, is
    booked).  callstate.h calls every result but OK / OVERFLOW / COVERAGE "refused", which holds for requested and covered but not for
    `device`: after such a call device > requested."""
    from ecloop_amd import capi
    hl = kc.OVER[1]
    k, want = kc.over_run()
    blk = kc.over_block()
    cap = len(want) + 64
    d = herd_device(0)
    try:
        d.reset_timing()
        cov = [d.coverage()]
        first, n1 = d.add_range(None, (k - 1) << hl, cap=cap, herd=blk)
        cov.append(d.coverage())
        with pytest.raises(capi.EclError) as e_next:
            d.add_range(None, 1 << hl, cap=cap, herd=blk)
        cov.append(d.coverage())
        s2 = d.setup_timing()[1]
        with pytest.raises(capi.EclError) as e_fresh:
            d.add_range(None, k << hl, cap=cap, herd=blk)
        cov.append(d.coverage())
        s3 = d.setup_timing()[1]
        again, n4 = d.add_range(None, (k - 1) << hl, cap=cap, herd=blk)
        cov.append(d.coverage())
        s4 = d.setup_timing()[1]
    finally:
        d.close()
    assert n1 == len(first) == len(want) and rec_set(first) == list(want)
    assert e_next.value.code == capi.E_RANGE and e_fresh.value.code == capi.E_RANGE
    assert n4 == len(again) and rec_set(again) == list(want) and (s2, s3, s4) == (1, 2, 3)
    whole = ((k - 1) << hl,) * 3
    assert [grown(a, b) for a, b in zip(cov, cov[1:])] == [whole, (0, 0, 1 << hl), (0, 0, k << hl), whole]


def test_end_to_end_at_a_wide_base():
    """W = 2^32 at a = 2^200 + 0x7000000000 (sc_add of a base above 2^128 in the set-up, the driver's B + d_t - d_w): the key and the statistics
    of the yardstick's driver"""
    from ecloop_amd import engine
    x, y = orc.point_of(kc.FAR_KEY)
    want_key, want = kc.far_search()
    got_key, got = engine.kangaroo_search("%02x%064x" % (2 | (y & 1), x), kc.FAR_A, kc.FAR_B, **kc.FAR_OPTIONS)
    print(got)
    assert want_key == kc.FAR_KEY == got_key and got == want
