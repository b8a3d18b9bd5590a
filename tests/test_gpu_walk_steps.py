"""The walk step of every `add` search kernel: the next centre C + J, its tangent branch (C == J), and the centres written back for a later
contiguous call - csrc/add_walk.inc lines 142-166, compiled separately into each kernel with a register allocation of its own.

Seventeen contexts (`c`, `u`, `cu`, `s`, `cs`, `us`, `cus` plain and with the endomorphism, `e` plain and with it, `t`; `c` is the control:
the addr33 kernel has these checks elsewhere, so a failure there points at this test), each on one Device through the shapes of
walk_ref.SHAPES at a caller-set geometry, where the automatic one would give every lane a single group:

  A  half group 8, 256 lanes, start 4056: lane 2's first centre is the jump point T * 2B * G, so its step is the tangent and its second,
     third and fourth group descend from it; 3 * 4096 + 5 keys: four rounds, the fourth with five live keys in lane 0 and none elsewhere.
  B  half group 2, the smallest, same construction (start 1014, 3 * 1024 + 3 keys).
  C  geometry A again: a call of one whole sweep (one round: the centres it stores are the step's first output, lane 2's from the
     tangent), then the contiguous call of 4096 + 5 keys that resumes from them - one positioning for the pair.

With the all-ones filter every call must report exactly {key offset x image x selected type}, each once, every record's 20 bytes equal to
tests/walk_ref.py's for calc_priv(start, 1, offset, image) - no key left out, nothing sampled, Taproot included - and the coverage totals
must grow by the call's keys.  Shape A is then repeated through a three-word filter of bit density 0.75 (no power of two words; keys pass
all twenty probes in rounds 2 to 4, so the rings' later stages run there): the records must be the all-ones expectation filtered by the
oracle's own test.  Taproot goes through the same twenty-probe filter, but in k_tr_check (tr_kernels.h: cand1_check on the leading 20
bytes of the output key), not in its walk kernel, which only leaves points in the slab: the filtered call checks that stage's rings and,
again, the walked points behind every record.  tests/test_walk_ref.py asserts on the CPU that the filtered expectation of every context is
non-empty.  Every assertion is an equality.

The prefix kernels (k_add_pfx, k_add_pfx_eth) reach the tangent nowhere else either - the (8, 256) calls of tests/test_gpu_prefix.py start
at 0x8000, above the jump point's scalar, and tests/test_gpu_splitkey.py walks from an origin - so shape A runs on a `c` and an `e` prefix
context too: through a table that takes every value, and through one made of the reference's values of the keys of lane 2's second and
third group alone.  The public-key kernels have theirs in tests/test_gpu_pub.py and tests/test_gpu_bsgs.py."""
import numpy as np
import pytest

import prefix_ref as R
import walk_ref
from synth import synth_bloom_words
from walk_ref import CONTEXTS, FILTER3, ONES, SHAPES, canon, difference, ref_of

pytestmark = pytest.mark.gpu


def checked_call(d, ref, name, first, count, what, wrong, filter3=None, want=None):
    """add_range over the keys first ... first + count - 1 of the reference's range: the records are the reference's, each once; the total
    is their number; the coverage totals grow by the call's keys.  What is not so goes to `wrong`, so that a failing context names every
    shape that fails (the tangent and the later rounds, or only the resumed call ...); -> the number of expected records"""
    want = ref.records(name, first, count, filter3) if want is None else want
    before = d.coverage()
    recs, total = d.add_range(ref.start + first, count, cap=len(want) + 16)
    grown = tuple(b - a for a, b in zip(before, d.coverage()))
    print("%s %s: %d records, %d expected, coverage +%s" % (name, what, total, len(want), grown))
    if not total == len(recs) == len(want):
        wrong.append("%s: a total of %d, %d records, %d expected" % (what, total, len(recs), len(want)))
    if difference(canon(recs), want) != "":
        wrong.append("%s: %s" % (what, difference(canon(recs), want)))
    if grown != (count, count, count):
        wrong.append("%s: coverage grew by %s for %d keys" % (what, grown, count))
    return len(want)


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_tangent_later_rounds_and_resumed_walk(name):
    from ecloop_amd import Device
    letters, endo, kw = CONTEXTS[name]
    per_key = len(letters) * (6 if endo else 1)
    wrong = []
    d = Device(0, **kw)
    try:
        d.set_bloom(ONES)
        for shape, (B, T, start, nkeys) in SHAPES.items():
            d.set_geometry(B, T)
            assert d.plan_geometry(nkeys) == (B, T, 4), (name, shape)
            assert checked_call(d, ref_of(shape), name, 0, nkeys, shape, wrong) == nkeys * per_key
        B, T, start, nkeys = SHAPES["A"]
        sweep = T * 2 * B
        d.set_geometry(B, T)
        assert d.plan_geometry(sweep) == (B, T, 1) and d.plan_geometry(sweep + 5) == (B, T, 2)
        positioned = d.setup_timing()[1]
        checked_call(d, ref_of("A"), name, 0, sweep, "C, the sweep", wrong)
        assert checked_call(d, ref_of("A"), name, sweep, sweep + 5, "C, resumed", wrong) == (sweep + 5) * per_key
        if d.setup_timing()[1] != positioned + 1:  # the second call has to go on from the centres the first one stored
            wrong.append("C: %d positionings for the pair of calls, 1 expected" % (d.setup_timing()[1] - positioned))
        d.set_bloom(synth_bloom_words(*FILTER3))
        assert checked_call(d, ref_of("A"), name, 0, nkeys, "A, three-word filter", wrong, FILTER3) > 0  # (the expectation: a condition on the inputs)
    finally:
        d.close()
    assert wrong == [], "%s: %s" % (name, "; ".join(wrong))


@pytest.mark.parametrize("name", ["c", "e"])
def test_prefix_kernels_take_the_tangent_too(name):
    from ecloop_amd import Device
    B, T, start, nkeys = SHAPES["A"]
    ref = ref_of("A")
    every = ref.records(name)
    own = [off for rnd in (1, 2) for off in walk_ref.group_offsets(B, T, 2, rnd)]  # lane 2's groups after the tangent
    values = sorted({R.value_of(r["h160"]) for r in every[np.isin(every["key_offset"], own)]})
    inside = R.membership([(v, v) for v in values])
    want = every[[inside(R.value_of(h)) for h in every["h160"].tolist()]]
    assert len(values) == 4 * B and len(want) >= len(values) and set(own) <= set(want["key_offset"].tolist())
    wrong = []
    d = Device(0, prefix=True, **CONTEXTS[name][2])
    try:
        d.set_geometry(B, T)
        assert d.plan_geometry(nkeys) == (B, T, 4)
        d.set_prefixes(np.array([R.words5(0) + R.words5(R.TOP)], np.uint32))
        checked_call(d, ref, name, 0, nkeys, "A, prefix, every value", wrong, want=every)
        d.set_prefixes(np.array([R.words5(v) + R.words5(v) for v in values], np.uint32).reshape(-1, 10))
        checked_call(d, ref, name, 0, nkeys, "A, prefix, lane 2's values", wrong, want=want)
    finally:
        d.close()
    assert wrong == [], "%s: %s" % (name, "; ".join(wrong))
