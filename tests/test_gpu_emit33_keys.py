"""The exact block of emit33_xwords (csrc/emit33.h) inside the addr33-only add kernels, on keys that take it.

emit33_xwords forms the SHA-256 message words of a compressed key straight from x's carried limbs, and goes through fe_normalize only
where limb 8 comes out at 2^24 - 1 or above: x has 24 leading one bits, 2^-24 per key and image - 256 keys of every 2^32-key call, and
none of any other test's.  tests/test_gpu_emit33.py runs the block on raw limbs (LIMB_EMIT33), a different compile; here it runs where
the search runs it: tests/golden/x_top24_keys.json (made by make_x_top24_keys.py, re-derived from the oracle in tests/test_digit_ref.py)
names keys whose x, beta x or beta^2 x has those bits.  Each key goes through three calls of 4096 + 5 keys at geometry (8, 256), the
start chosen so that it is a lane's centre (x comes from the centre's limbs), a member C + G_5, and a member C - G_6 of the ragged second
round (x = lam^2 - X - Gx at magnitude 4): on k_add<true, false, true> every key (the images are x's multiples by beta, formed in
check_point33), on k_add<true, false, false> the keys whose own x it is.  All-ones filter: every record of every call against
tests/walk_ref.py, and the coverage totals whole - a wrong word in the block is another hash for that key alone."""
import functools
import json
import os

import pytest

import walk_ref
from test_gpu_walk_steps import checked_call

pytestmark = pytest.mark.gpu
B, T = 8, 256
NKEYS = T * 2 * B + 5
POSITIONS = {"centre": 37 * 2 * B + B, "C + G_5": 200 * 2 * B + B + 5, "C - G_6": T * 2 * B + B - 6}  # the key's offset in its call
SPAN = max(POSITIONS.values()) - min(POSITIONS.values()) + NKEYS  # keys of the reference that serves a key's three calls
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x_top24_keys.json")) as f:
    ROWS = json.load(f)["rows"]


def ref_start(key):
    return key - max(POSITIONS.values())


def first_of(pos):
    """where in the reference's range the call begins that has the key at offset `pos`"""
    return max(POSITIONS.values()) - pos


@functools.lru_cache(maxsize=2)
def ref_of(key):
    return walk_ref.WalkRef(ref_start(key), SPAN)


@pytest.mark.parametrize("row", ROWS, ids=["%d-beta%d" % (r["key"], r["image"]) for r in ROWS])
def test_a_key_with_24_leading_one_bits_in_three_positions(row):
    from ecloop_amd import Device
    key, image = row["key"], row["image"]
    ref = ref_of(key)
    wrong = []
    for name in ("c-endo", "c") if image == 0 else ("c-endo",):
        d = Device(0, **walk_ref.CONTEXTS[name][2])
        try:
            d.set_geometry(B, T)
            d.set_bloom(walk_ref.ONES)
            assert d.plan_geometry(NKEYS) == (B, T, 2)
            for what, pos in POSITIONS.items():
                n = checked_call(d, ref, name, first_of(pos), NKEYS, "%s, %s" % (name, what), wrong)
                assert n == NKEYS * (6 if name == "c-endo" else 1)
        finally:
            d.close()
    assert wrong == [], "%d: %s" % (key, "; ".join(wrong))
