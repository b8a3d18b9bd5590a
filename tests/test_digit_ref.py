"""tests/digit_ref.py - the signed window recoding restated - against hand-worked values, and the conditions on their inputs that the
zero-digit GPU tests rely on, checked here on the CPU: the fixtures tests/golden/tr_zero_digit_points.json and x_top24_keys.json row by
row, the tweaks of walk_ref's shape A at the narrow widths (tests/test_gpu_tr_digits.py), the threads of mul_ref's shape A whose two
scalars - and, on a Taproot context, whose two tweaks - take the complete sum in both rounds or in one (tests/test_gpu_mul_types.py), and
the three positions of a key in a call of tests/test_gpu_emit33_keys.py."""
import json
import os
import random

import numpy as np
import pytest

import digit_ref as D
import mul_ref
import orc
import tr_ref
import walk_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M256 = (1 << 256) - 1


def fill(W, **digits):
    """the scalar whose raw digit is 1 in every window but those named: fill(8, w3=0xFF)"""
    d = {w: 1 for w in range(D.windows(W))}
    d.update({int(k[1:]): v for k, v in digits.items()})
    return sum(v << (W * w) for w, v in d.items())


# worked by hand from the rule: v = raw + carry; v > 2^(W-1) below the last window: the digit is v - 2^W, and 1 is carried
HAND = [
    (fill(8), 8, []),
    (fill(8, w0=0), 8, [(0, "raw0")]),
    (fill(8, w1=0), 8, [(1, "raw0")]),
    (fill(8, w1=0, w2=0), 8, [(1, "raw0"), (2, "raw0")]),
    (fill(8, w0=0x80, w1=0xFF), 8, []),                    # 0x80 stays positive; 0xFF is -1 and carries: window 2 is 2
    (fill(8, w0=0x81, w1=0xFF), 8, [(1, "carry")]),        # 0x81 is -0x7F and carries: window 1 is 0x100 = 0 and carries on
    (fill(8, w0=0x81, w1=0xFF, w2=0xFF), 8, [(1, "carry"), (2, "carry")]),
    (fill(8, w1=0xFF, w2=0), 8, []),                       # a raw zero that the carry fills
    (fill(8, w17=0x81, w18=0xFF), 8, [(18, "carry")]),
    (fill(8, w30=0x7F, w31=0), 8, [(31, "raw0")]),         # the last window: t < 2^248 without a carry into it
    (fill(8, w30=0x81, w31=0), 8, []),                     # ... with one
    (fill(8, w30=0x81, w31=0xFF), 8, []),                  # the last window is not recoded: 0x100 is slot 256 of its row
    (fill(22, w11=0), 22, [(11, "raw0")]),                 # 22 bits: twelve windows, the last one 14 bits; t < 2^242
    (fill(22, w10=(1 << 21) + 1, w11=0), 22, []),
    (fill(22, w10=1 << 21, w11=0), 22, [(11, "raw0")]),    # exactly 2^(W-1) stays positive
    (fill(26, w4=(1 << 25) + 1, w5=(1 << 26) - 1), 26, [(5, "carry")]),
    (fill(13, w18=(1 << 13) - 1, w19=(1 << 9) - 1), 13, []),  # 13 bits: twenty windows, the last one 9 bits: 2^9 - 1 + 1 is slot 2^9
    (1, 8, [(w, "raw0") for w in range(1, 32)]),
    (0, 26, [(w, "raw0") for w in range(10)]),
    (M256, 22, [(w, "carry") for w in range(1, 11)]),      # -1 in window 0, then ten times 2^W = 0; the last window is 2^14, a slot
]


def test_zero_digits_on_hand_worked_values():
    assert len(HAND) >= 12
    for t, W, want in HAND:
        assert D.zero_digits(t, W) == want, (hex(t), W)
    assert [D.windows(W) for W in (8, 11, 13, 22, 26)] == [32, 24, 20, 12, 10]
    assert [D.window_class(w, 22) for w in range(12)] == ["w0", "w1", "w2"] + ["middle"] * 8 + ["top"]


def test_signed_digits_sum_to_the_scalar_and_stay_in_range():
    rng = random.Random(8)
    for W in D.WIDTHS + (14, 29):
        n = D.windows(W)
        for t in [rng.getrandbits(256) for _ in range(200)] + [0, 1, M256, orc.N, orc.N - 1] + [h[0] for h in HAND]:
            ds = D.signed_digits(t, W)
            assert sum(d << (W * w) for w, (d, _) in enumerate(ds)) == t
            assert all(-(1 << (W - 1)) < d <= 1 << (W - 1) for d, _ in ds[:-1]) and 0 <= ds[-1][0] <= 1 << (256 - W * (n - 1))
            assert D.zero_digits(t, W) == [(w, "carry" if c else "raw0") for w, (d, c) in enumerate(ds) if d == 0]


def test_the_loop_bound_of_a_wave():
    """wtab_sum_fast: windows above every lane's bits are cut, never below two; a lane of (nw - 1) W bits keeps window nw - 1 (bit (nw - 1) W - 1 may carry into it)"""
    assert D.windows_walked([1, 2, 3], 22) == 2 and D.windows_walked([1, 1 << 42], 22) == 2 and D.windows_walked([1, 1 << 43], 22) == 3
    assert D.windows_walked([1, 1 << 240], 22) == 11 and D.windows_walked([1 << 241, 5], 22) == 12 and D.windows_walked([M256], 8) == 32
    t = fill(22, w11=0)
    assert D.flagged(t, [t, M256], 22) == [(11, "raw0")] and D.flagged(t, [t, t], 22) == []  # alone, the wave never walks window 11
    assert D.flagged(1 << 100, [1 << 100, M256], 22) == [(w, "raw0") for w in range(12) if w != 4]


# ---------------------------------------------------------------------------------------------- the fixtures
def tr_rows():
    with open(os.path.join(GOLD, "tr_zero_digit_points.json")) as f:
        return [dict(r, x=int(r["x"], 16), y=int(r["y"], 16)) for r in json.load(f)["rows"]]


def top24_rows():
    with open(os.path.join(GOLD, "x_top24_keys.json")) as f:
        return json.load(f)["rows"]


def test_every_fixture_point_is_on_the_curve_and_its_tweak_has_the_named_zero_digit():
    rows = tr_rows()
    for r in rows:
        assert 0 < r["x"] < orc.P and 0 < r["y"] < orc.P and (r["y"] * r["y"] - r["x"] ** 3 - 7) % orc.P == 0
        t = tr_ref.tweak(r["x"])
        assert t < orc.N and (r["window"], r["cause"]) in D.zero_digits(t, r["W"]), r
    for W in (22, 26):
        mine = [r for r in rows if r["W"] == W]
        assert {D.window_class(r["window"], W) for r in mine} == set(D.CLASSES), W  # window 0, 1, 2, a middle one, the top one
        assert any(r["cause"] == "carry" for r in mine) and any(r["cause"] == "raw0" for r in mine), W
        assert {r["y"] & 1 for r in mine} == {0, 1}  # both lifts
    assert len({r["x"] for r in rows}) == len(rows)


def test_every_fixture_key_has_24_leading_one_bits_in_the_named_image():
    rows = top24_rows()
    for r in rows:
        x = orc.point_of(r["key"])[0] * pow(walk_ref.BETA, r["image"], orc.P) % orc.P
        assert x >= (1 << 256) - (1 << 232) and x == int(r["x"], 16), r
    count = [sum(r["image"] == i for r in rows) for i in range(3)]
    assert count[0] >= 3 and count[1] >= 2 and count[2] >= 2
    assert len({r["key"] for r in rows}) == len(rows)


def test_the_three_positions_of_a_key_in_a_call():
    """tests/test_gpu_emit33_keys.py: the key as a lane's centre, as C + G_i and as C - G_i (add_walk.inc: a group's keys are base ...
    base + 2B - 1, the centre base + B, C + G_i at base + B + i, C - G_i at base + B - i), the last in the ragged second round"""
    import test_gpu_emit33_keys as E
    B, T = E.B, E.T
    assert (B, T, E.NKEYS) == (8, 256, 4096 + 5) and len(E.POSITIONS) == 3
    kinds = set()
    for what, pos in E.POSITIONS.items():
        assert 0 <= pos < E.NKEYS
        rnd, lane, k = pos // (T * 2 * B), pos // (2 * B) % T, pos % (2 * B)
        assert pos in walk_ref.group_offsets(B, T, lane, rnd)
        kinds.add((what, "centre" if k == B else "plus" if k > B else "minus", rnd))
    assert kinds == {("centre", "centre", 0), ("C + G_5", "plus", 0), ("C - G_6", "minus", 1)}
    for r in top24_rows():
        for pos in E.POSITIONS.values():
            first = E.first_of(pos)
            assert 0 <= first and first + E.NKEYS <= E.SPAN and E.ref_start(r["key"]) + first + pos == r["key"]


# ---------------------------------------------------------------------------------------------- shape A of walk_ref at narrow widths
# keys with a zero digit; digits in window 0 / 1 / 2 / a middle window / the top window; digits by carry / raw zero; keys with more than one
COUNTS = {8: (1398, (56, 47, 52, 1278, 42), (689, 786), 74), 11: (857, (6, 6, 6, 119, 734), (61, 810), 14), 13: (54, (2, 3, 3, 25, 21), (13, 41), 0),
          22: (3, (0, 0, 0, 0, 3), (0, 3), 0), 26: (0, (0, 0, 0, 0, 0), (0, 0), 0)}
_tweaks = {}


def shape_a_tweaks():
    if not _tweaks:
        _, _, start, nkeys = walk_ref.SHAPES["A"]
        _tweaks["A"] = [tr_ref.tweak(orc.point_of(start + off)[0]) for off in range(nkeys)]
    return _tweaks["A"]


@pytest.mark.parametrize("W", sorted(COUNTS))
def test_zero_digit_tweaks_of_shape_a(W):
    """what k_tr_check meets in the Taproot calls over walk_ref's shape A: at 22 bits three keys, all in the top window; at 26 none; at
    8, 11 and 13 bits (tests/test_gpu_tr_digits.py) every class of window, both causes and - at 8 - several digits in one tweak.  A
    launch of 12 293 entries has one key per thread, entry i in thread i: a wave is 64 consecutive keys, and every digit counted here
    lies below its wave's loop bound"""
    B, T, start, nkeys = walk_ref.SHAPES["A"]
    ts = shape_a_tweaks()
    assert mul_ref.geometry(nkeys) == (1, 12544)
    zs = [D.zero_digits(t, W) for t in ts]
    assert all(D.flagged(t, ts[i // 64 * 64:i // 64 * 64 + 64], W) == zs[i] for i, t in enumerate(ts) if zs[i])
    digits = [(D.window_class(w, W), cause) for z in zs for w, cause in z]
    got = (sum(1 for z in zs if z), tuple(sum(c == k for c, _ in digits) for k in D.CLASSES),
           tuple(sum(c == k for _, c in digits) for k in ("carry", "raw0")), sum(1 for z in zs if len(z) > 1))
    assert got == COUNTS[W]
    if W == 22:
        assert [start + i for i, z in enumerate(zs) if z] == [7679, 8318, 8836]
    if W in (8, 13):  # the conditions of the GPU test
        assert all(n > 0 for n in got[1])
    if W == 8:
        assert all(n > 0 for n in got[2]) and got[3] > 0
        passes = walk_ref.ref_of("A").passes("tr", walk_ref.FILTER3)[:, 0]
        assert sum(1 for i, z in enumerate(zs) if z and passes[i]) > 0  # a complete-sum key among the filtered call's records


# ---------------------------------------------------------------------------------------------- shape A of mul_ref at 8 bits
def rounds_of_threads(values, live):
    """values[i]: the scalar (or tweak) of entry i of a launch of NA entries, two per thread; live[i]: whether it is known.  -> the
    numbers of threads, both of whose entries are known, that take the complete sum in both rounds, in round 0 only, in round 1 only"""
    R, nt = mul_ref.geometry(mul_ref.NA)
    assert (R, nt) == (2, 131328)
    sure = [False] * mul_ref.NA  # flagged for certain: a zero digit below the bound that the wave's known lanes alone set
    for at in range(0, mul_ref.NA, 64):  # nt is a multiple of 64: a wave's lanes are 64 consecutive entries of one round
        lanes = [i for i in range(at, min(at + 64, mul_ref.NA)) if live[i]]
        wave = [values[i] for i in lanes]
        for i in lanes:
            sure[i] = bool(D.flagged(values[i], wave, 8))
    clean = lambda i: live[i] and not D.zero_digits(values[i], 8)
    both = r0 = r1 = 0
    for t in range(mul_ref.NA - nt):  # the threads with two entries
        a, b = t, nt + t
        both += sure[a] and sure[b]
        r0 += sure[a] and clean(b)
        r1 += clean(a) and sure[b]
    return both, r0, r1


def test_threads_of_mul_shape_a_with_the_complete_sum_in_both_rounds_and_in_one():
    """tests/test_gpu_mul_types.py at 8 bits: a thread's product chain with the out-of-line sum in both of its rounds, in the first
    alone, in the second alone - over the scalars (every mul kernel), and over the tweaks of their points (k_tr_check on context `t`)"""
    K, _ = mul_ref.scalars()
    ks = mul_ref.ints_of(K[:mul_ref.NA])
    got = rounds_of_threads(ks, [True] * mul_ref.NA)
    print("scalars: both rounds %d, round 0 only %d, round 1 only %d" % got)
    assert min(got) > 0
    r = mul_ref.ref()
    ok = r.ok[:mul_ref.NA].tolist()
    xs = mul_ref.ints_of(r.points[0][:mul_ref.NA])
    ts = [tr_ref.tweak(x) if o else 0 for x, o in zip(xs, ok)]
    got = rounds_of_threads(ts, ok)
    print("tweaks: both rounds %d, round 0 only %d, round 1 only %d" % got)
    assert min(got) > 0
    assert np.count_nonzero(~r.ok[:mul_ref.NA]) > 0  # (entries without a point: their slab entry's tweak is not known here, and is not counted)
