"""The set-up kernels of a non-contiguous `add` call (csrc/setup_kernels.h) at the lane counts the product runs, lane by lane, and single
calls of more than 2^32 keys - through a filter that holds nothing but planted keys (tests/lane_ref.py), so that a call of 2^21 ... 2^33
keys is checked exactly: its records must be the planted set, each once.

  a  8 x 2^19 lanes: k_init_centres_table<8> with E on the table point of a lane in slot r = 0, 3, 4, 7 of the first, a middle and the last
     thread - the exceptional lane, the other seven of its thread, the seams between threads
  b  8 x 2^18 lanes: the same for <4> at the largest lane count it serves
  c  8 x 2^19, E = infinity (k_init_centres_batched from C0), start 9, a 200-bit start: the ladder up to 2^18 D
  d  2 x 2^19: k_init_centres (half group below 8) builds the table, <8> behind it
  e  16 x 2^19 at stride 2^13
  f  the automatic geometry of 2^30 keys (2^21 lanes) from an exceptional start
  g  an origin in front of the set-up: E + O on a table point (k_origin_add, then <8>), and the next origin on the same context
  h  one call of 2^32 + 2^22 + 5 keys: several rounds per lane, key offsets past 2^32
  i  the same past the caller's cap: the rest through fetch_found

Every assertion on the device's answer is an equality.  The planted lanes, offsets, the filter's conditions and the reference are checked
on the CPU by tests/test_lane_ref.py."""
import numpy as np
import pytest

import lane_ref
import orc
import walk_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(lane_ref.CASES))
def test_lane_centres_and_offsets_through_a_planted_filter(name):
    from ecloop_amd import Device
    case = lane_ref.CASES[name]
    failures = []
    d = Device(0, **case.device)
    try:
        if case.geometry:
            d.set_geometry(*case.geometry)
            B, T, nb = case.geometry + (1,)
        else:  # the automatic geometry: read, and checked against the arithmetic it stands for
            B, T, nb = d.plan_geometry(case.nkeys)
            assert (T, nb) == lane_ref.lanes_and_rounds(case.nkeys, B, d.geometry()[1])
        for call in case.calls(B, T, nb):
            want = case.expected(call, B, T, nb)
            if name in "hi":  # conditions on the inputs: rounds at full lane count, offsets that need more than 32 bits
                assert nb >= 2 and int((want["key_offset"] >= 1 << 32).sum()) >= 100
            d.set_bloom(lane_ref.planted_filter(want["h160"]))
            assert d.plan_geometry(case.nkeys) == (B, T, nb)  # the path under test is the one taken
            cov, ups = d.coverage(), d.setup_timing()[1]
            recs, total = d.add_range(call.start, case.nkeys, cap=case.cap, origin=None if call.t is None else orc.point_of(call.t))
            grown = tuple(b - a for a, b in zip(cov, d.coverage()))
            positioned = d.setup_timing()[1] - ups
            if name == "i":  # past the cap: the total is the planted count, the call delivered `cap`, the rest is still on the device
                if (total, len(recs)) != (len(want), case.cap):
                    failures.append("%s: total %d with %d delivered, %d and %d expected" % (call.label, total, len(recs), len(want), case.cap))
                recs = np.concatenate([recs, d.fetch_found(len(recs), max(total, 1))])
            got = walk_ref.canon(recs)
            diff = walk_ref.difference(got, want)
            if diff:
                failures.append("%s (start %x, exceptional lane %s): %s; lanes that differ: %s"
                                % (call.label, call.start, call.m, diff, lane_ref.lanes_that_differ(got, want, B, T)))
            if total != len(recs):
                failures.append("%s: total %d, %d records" % (call.label, total, len(recs)))
            if len(recs) and int(recs["key_offset"].max()) >= case.nkeys:
                failures.append("%s: key offset %d in a call of %d keys" % (call.label, int(recs["key_offset"].max()), case.nkeys))
            if grown != (case.nkeys,) * 3:
                failures.append("%s: the coverage totals grew by %s" % (call.label, grown))
            if positioned != 1:
                failures.append("%s: %d set-ups" % (call.label, positioned))
    finally:
        d.close()
    assert len(failures) == 0, "\n".join(failures)
