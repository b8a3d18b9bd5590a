"""k_tr_check's out-of-line complete sum (csrc/tr_kernels.h: tr_sum_complete) on tweaks that need it.

Stage B of Taproot sums t G by wtab_sum_fast over the digits of the tweak t.  A signed digit of magnitude zero takes a stand-in table
point and flags the key, which is then summed again by the complete formulas inside the loop that builds the thread's product chain - a
wrong result there is one key silently missed.  t is a SHA-256 output and cannot be planted; at the 22-bit table the keys of the other
Taproot tests hold a handful of such tweaks, all in the top window, and at 26 bits none.  Two ways to the rest:

  * the width is a run-time choice that Taproot contexts honour.  walk_ref's shape A (geometry (8, 256), four rounds, the tangent in
    lane 2) at 8, 11 and 13 bits: of its 12 293 tweaks 1398 / 857 / 54 hold a zero digit - in window 0 and 1 (the affine + affine
    start), in window 2 (fetched ahead of the loop), in middle windows, in the top one, made by a raw zero and by a carry, and at 8 bits
    74 tweaks hold several.  The records must be walk_ref's for context `t`, which do not depend on the width; at 8 bits again through
    the three-word filter (cand1_check behind the complete sum).
  * at the production widths, points found for the purpose: tests/golden/tr_zero_digit_points.json (make_tr_zero_digit_points.py) holds
    curve points whose tweak has a zero digit in window 0, 1, 2, a middle and the top window and one made by a carry, for 22 and for 26
    bits.  ecl_hip_diag_tr takes any affine point: they go through k_tr_check<true> among 4096 of the oracle's points; tweak, output
    key and flag of every point against tests/tr_ref.py.

tests/test_digit_ref.py asserts on the CPU, with the recoding restated in tests/digit_ref.py, that the inputs hold what is said here."""
import json
import os

import pytest

import orc
import tr_ref
from synth import synth_bloom_words
from test_gpu_walk_steps import checked_call
from walk_ref import CONTEXTS, FILTER3, ONES, SHAPES, ref_of

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("W", [8, 11, 13])
def test_taproot_walk_at_narrow_widths(W):
    from ecloop_amd import Device
    B, T, start, nkeys = SHAPES["A"]
    ref = ref_of("A")
    wrong = []
    d = Device(0, **CONTEXTS["t"][2])
    try:
        d.set_geometry(B, T)
        d.set_mul_window(W)
        d.set_bloom(ONES)
        assert d.plan_geometry(nkeys) == (B, T, 4)
        assert checked_call(d, ref, "t", 0, nkeys, "A, W = %d" % W, wrong) == nkeys
        if W == 8:
            d.set_bloom(synth_bloom_words(*FILTER3))
            assert checked_call(d, ref, "t", 0, nkeys, "A, W = 8, three-word filter", wrong, FILTER3) > 0
        assert d.mul_window() == W
    finally:
        d.close()
    assert wrong == [], "W = %d: %s" % (W, "; ".join(wrong))


NPOINTS, FIRST_KEY = 4096, 0x7A3000  # the oracle's points the fixture's are mixed into


@pytest.mark.parametrize("W", [22, 26])
def test_points_whose_tweak_has_a_zero_digit_at_a_production_width(W):
    from ecloop_amd import Device
    with open(os.path.join(GOLD, "tr_zero_digit_points.json")) as f:
        rows = [r for r in json.load(f)["rows"] if r["W"] == W]
    assert len(rows) >= 5
    mine = [(int(r["x"], 16), int(r["y"], 16)) for r in rows]
    n = NPOINTS + len(mine)
    step = (n - 1) // (len(mine) - 1)
    planted = [j * step for j in range(len(mine) - 1)] + [n - 1]  # lane 0 of the first wave, other waves and lanes, the last lane of all
    oracle = (orc.point_of(FIRST_KEY + i) for i in range(NPOINTS))
    pts = [mine[planted.index(i)] if i in planted else next(oracle) for i in range(n)]
    d = Device(0, **CONTEXTS["t"][2])
    try:
        d.set_mul_window(W)
        t, qx, ok = d.diag_tr([p[0] for p in pts], [p[1] for p in pts])
        assert d.mul_window() == W
    finally:
        d.close()
    want = [tr_ref.output_key_of_point(*p) for p in pts]
    assert None not in want
    assert t == [tr_ref.tweak(p[0]) for p in pts]
    assert ok.tolist() == [1] * len(pts)
    bad = [i for i, q in enumerate(want) if qx[i].tolist() != tr_ref.words8(q)]
    assert bad == [], "%d output keys differ, at %s; the fixture's points are at %s" % (len(bad), bad[:8], planted)
