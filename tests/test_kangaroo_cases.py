"""The inputs of tests/test_gpu_kangaroo_wide.py (tests/kangaroo_cases.py) have the properties they were made for: asserted here without a
GPU, on the yardstick alone, so that a GPU test that passes has passed on the path it names."""
import os

import numpy as np
import pytest

import kangaroo_cases as kc
import kangaroo_ref as ref
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, N = orc.P, orc.N


@pytest.mark.parametrize("name", list(kc.WIDE))
def test_wide_cases_use_the_upper_words(name):
    """the records hold distances with word 2 and with word 3 in use, recorded jumps in which word 1 carried into word 2, and the table has
    distances of 2^64 and more (rows 20, 21 of the kernel's table); the base is wider than 128 bits"""
    hl, seed, jb, sb, dp, steps = kc.WIDE[name]
    recs, seen = kc.wide_run(name)
    print(name, len(recs), seen)
    assert kc.WIDE_BASE >> 128 and len(recs) > 0 and all(r[3] == 6 for r in recs)
    assert seen["word2"] > 0 and seen["carry"] > 0 and seen["table_hi"] > 0
    if sb > 96:
        assert seen["word3"] > 0 and any(s >> 96 for s in ref.distances_and_offsets(seed, hl, jb, sb)[1])
    else:  # (jb = sb = 64, dp = 0: every jump is a record, the case of the 2^64 carry; word 3 is the other cases')
        assert dp == 0 and len(recs) == steps << hl and seen["carry"] > steps
    # the packing: words 2 and 3 of a distance are h160[1] and h160[0]
    assert any(r[1][1] != r[1][0] and ref.distance_of(r) >> 64 == (r[1][0] << 32 | r[1][1]) for r in recs)


@pytest.mark.parametrize("name", list(kc.DP_TARGETS))
def test_dp_targets_put_one_point_on_the_limb_boundary(name):
    """wild kangaroo 1 starts on X* - T_j, picks j, and its first jump lands on X*, whose x has exactly the low bits of the name; over the 8
    steps the yardstick expects that one record at the dps that take it and none at the next dp"""
    z, top, runs = kc.DP_TARGETS[name]
    blk, j, star = kc.dp_target(name)
    base, q, seed, hl, jb, sb = blk
    s, r = ref.distances_and_offsets(seed, hl, jb, sb)
    T = [orc.point_of(v) for v in s]
    assert (star[1] * star[1] - star[0] ** 3 - 7) % P == 0 and (q[1] * q[1] - q[0] ** 3 - 7) % P == 0
    assert star[0] & ((1 << z) - 1) == 0 and bool(star[0] >> z & 1) == top and star[0] >> 64  # random above the low bits
    start = ref.start_of(base, q, r[1], 1)
    assert (start[0] >> 32) & 31 == j and start[0] != T[j][0] and ref.jump_of(s, T, start, r[1]) == (j, star, r[1] + s[j])
    herd = ref.Herd(*blk)
    assert (herd.x[1], herd.y[1]) == start
    first = ref.record(1, r[1] + s[j], star[0])
    assert ref.distance_of(first) == r[1] + s[j] and first[2] == 1
    for dp, expected in runs:
        assert list(kc.dp_run(name, dp)) == ([first] if expected else []), (name, dp)
        assert (star[0] & ((1 << dp) - 1) == 0) == expected
    assert first in ref.Herd(*blk).step(dp=runs[0][0])  # ... and it is the first step's
    # between them the runs cross bit 29, where limb 1 of x begins: a dp of 30 or more is decided there
    assert any(dp >= 30 for dp, _ in kc.DP_TARGETS["Z32"][2]) and {dp for t in kc.DP_TARGETS.values() for dp, _ in t[2]} == {28, 29, 30, 31, 32}


def test_long_calls_cross_the_launch_cap():
    """H2 is three launches (4096 + 4096 + 7 steps), H32 two (4096 + 1); the split of H2 is two calls of two launches each"""
    cap = kc.LAUNCH_STEPS_MAX
    src = open(os.path.join(ROOT, "ecloop_amd", "csrc", "abi_herd.h")).read()
    assert "#define HERD_LAUNCH_STEPS_MAX %du" % cap in src and "#define HERD_INIT_CHUNK (1u << 18)" in src and kc.INIT_CHUNK == 1 << 18
    assert kc.LONG["H2"][0] == 1 and kc.LONG["H2"][5] == 2 * cap + 7 and kc.LONG["H32"][0] == 5 and kc.LONG["H32"][5] == cap + 1
    assert sum(kc.LONG_SPLIT) == kc.LONG["H2"][5] and all(cap < v < 2 * cap for v in kc.LONG_SPLIT)
    for name in kc.LONG:
        hl, _, _, _, dp, steps = kc.LONG[name]
        recs = kc.long_run(name)
        print(name, len(recs))
        assert (steps << hl) >> (dp + 1) < len(recs) < (steps << hl) >> (dp - 1)  # about one jump in 2^dp


def test_the_two_chunk_herd_is_unambiguous():
    """2^19 kangaroos are two set-up chunks; the offsets are distinct, the sums r_i + s_j are distinct within each herd, so a record's distance
    names its kangaroo and its jump; every distance is below 2^63"""
    hl, seed, jb, sb = kc.BIG
    s, r = kc.big_herd()
    H = 1 << hl
    assert H == 2 * kc.INIT_CHUNK and len(r) == H and len(set(r)) == H
    assert max(r) + max(s) < 1 << 63
    S = np.array(s, np.uint64)
    for par in (0, 1):
        R = np.array(r[par::2], np.uint64)
        sums = (R[:, None] + S[None, :]).ravel()
        assert len(sums) == 32 * H // 2 and len(np.unique(sums)) == len(sums)
    sample = kc.big_sample()
    assert len(sample) == len(set(sample)) == 64 and sample[:10] == [0, 1, 2, 3, (1 << 18) - 2, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, H - 2, H - 1]
    assert any(i < kc.INIT_CHUNK for i in sample[10:]) and any(i >= kc.INIT_CHUNK for i in sample[10:])
    want = kc.big_expected()
    assert sorted(want) == sorted(sample) and all(rec[2] == i & 1 and rec[3] == 6 for i, rec in want.items())
    assert all(ref.distance_of(want[i]) - r[i] in s for i in sample)


def test_the_odd_starts_and_the_overflow_are_what_they_claim():
    # a start at infinity, wild and tame: the yardstick raises
    for blk in (kc.wild_infinity_block(), kc.tame_infinity_block()):
        with pytest.raises(ValueError):
            ref.Herd(*blk)
    base, q, seed, hl, jb, sb = kc.wild_infinity_block()
    r = ref.distances_and_offsets(seed, hl, jb, sb)[1]
    assert r[1] and ref.start_of(base, q, r[1], 1) is None and (q[1] * q[1] - q[0] ** 3 - 7) % P == 0
    base, q, seed, hl, jb, sb = kc.tame_infinity_block()
    assert 0 < base < N and ref.start_of(base, q, r[0], 0) is None
    assert len(kc.odd_good_run()) > 0
    # zero offsets on both herds: the wild start is Q itself, the tame one base G; equal offsets walk together, so records repeat
    base, q, seed, hl, jb, sb = kc.zero_block()
    r = ref.distances_and_offsets(seed, hl, jb, sb)[1]
    assert set(r) == {0, 1} and 0 in r[0::2] and 0 in r[1::2]
    herd =ref.Herd(base, q, seed, hl, jb, sb)
    wild0 = [k for k in range(1, len(r), 2) if r[k] == 0]
    tame0 = [k for k in range(0, len(r), 2) if r[k] == 0]
    assert all((herd.x[k], herd.y[k]) == tuple(q) for k in wild0) and all((herd.x[k], herd.y[k]) == orc.point_of(base) for k in tame0)
    recs = kc.zero_run()
    assert len(recs) == kc.ZERO[5] << hl and len(set(recs)) < len(recs)
    # the overflow: step k raises, 2 <= k <= 600, and the k - 1 steps before it use all four words of the distance
    k, recs = kc.over_run()
    print("overflow at step", k)
    assert 2 <= k <= 600 and len(recs) == (k - 1) << kc.OVER[1]
    herd = ref.Herd(*kc.over_block())
    herd.run(k - 1, 0)
    with pytest.raises(OverflowError):
        herd.step(0)
    assert all(any(kc.words_of(ref.distance_of(rec))[w] for rec in recs) for w in range(4))
    assert any(ref.distance_of(rec) >> 127 for rec in recs)


def test_the_far_search_finds_its_key():
    """W = 2^32 at a = 2^200 + 0x7000000000: the yardstick's driver finds the key; the plan is the one of the same width at a small base"""
    key, stats = kc.far_search()
    near = ref.plan(0x7000000000, 0x7000000000 + (1 << 32) - 1, 8, 5)
    far = ref.plan(kc.FAR_A, kc.FAR_B, 8, 5)
    assert key == kc.FAR_KEY and kc.FAR_A < key < kc.FAR_B and kc.FAR_A >> 200 == 1
    assert {k: v for k, v in far.items() if k != "base"} == {k: v for k, v in near.items() if k != "base"} and far["base"] == kc.FAR_A
    assert stats["rounds"] >= 1 and stats["candidates_checked"] >= 1
