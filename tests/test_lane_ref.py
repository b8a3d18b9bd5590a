"""tests/lane_ref.py, the reference of tests/test_gpu_lane_setup.py, on the CPU: the exceptional start against its definition, the lanes
of interest against their list, the planted offsets and the filter of every case against the conditions that make set equality sound,
and two expected records per call re-derived from the oracle's point."""
import numpy as np
import pytest

import lane_ref
import orc
import pub_ref
import walk_ref

# the automatic cases also on a device whose memory is short (half the lanes: one round more)
PLANS = [(name, None) for name in lane_ref.CASES] + [(name, 1 << 20) for name, c in lane_ref.CASES.items() if c.geometry is None]


def test_exceptional_start_against_the_definition():
    for B in (2, 8, 16, 256, 1024):
        for offs in (0, 1, 13):
            s = 1 << offs
            for T in (256, 1 << 18, 1 << 19, 1 << 21):
                for m in (0, 1, 5, T // 8 * 7 + 5, T - 1):
                    start = lane_ref.exceptional_start(B, offs, m)
                    assert start + B * s - 2 * B * s == (m + 1) * 2 * B * s  # E = C0 - D is the table point (m + 1) D of lane m
                    assert walk_ref.centre(start // s, B, T, m) * s == 2 * (m + 1) * 2 * B * s  # ... whose centre is its double
    assert lane_ref.exceptional_start(8, 0, 5) == 16 * 5 + 24  # the start of tests/test_gpu_add.py's case at 256 lanes


@pytest.mark.parametrize("T", [1 << 18, 1 << 19, 1 << 21])
def test_lanes_of_interest_hold_the_seams_the_ladder_bits_and_the_exceptional_thread(T):
    per = lane_ref.per_thread_of(T)
    assert per == (4 if T < 1 << 19 else 8)
    nt = T // per
    m = (per - 3) * nt + 77
    plain, lanes = lane_ref.lanes_of_interest(T, per), lane_ref.lanes_of_interest(T, per, m)
    assert lanes == sorted(set(lanes)) and plain == sorted(set(plain)) and set(plain) < set(lanes)
    assert lanes[0] == 0 and lanes[-1] == T - 1
    want = {0, 1, T - 1, nt - 1, nt, nt + 1}
    want |= {r * nt for r in range(per)} | {r * nt + nt - 1 for r in range(per)}
    want |= {g for j in range(1, 32) if 1 << j < T for g in ((1 << j) - 1, 1 << j, (1 << j) + 1)}
    assert want <= set(plain)
    assert T // 2 in plain  # the ladder's top bit
    assert len([g for g in plain if g % 16 == 15 and g + 1 in plain]) >= 8  # seams of the batched kernel, both sides
    assert len(set(plain) - want) >= 64  # the seeded lanes (and the sixteens)
    assert plain == lane_ref.lanes_of_interest(T, per)  # seeded: the same every time
    assert {m - 1, m, m + 1} <= set(lanes) and {r * nt + m % nt for r in range(per)} <= set(lanes)
    assert len([g for g in lanes if g % nt == m % nt]) >= per
    assert len(lanes) < 300


@pytest.mark.parametrize("name,Tmax", PLANS)
def test_planted_offsets_stay_inside_the_call_and_below_the_cap(name, Tmax):
    case = lane_ref.CASES[name]
    B, T, nb = case.plan(Tmax)
    assert (nb - 1) * T * 2 * B < case.nkeys <= nb * T * 2 * B and T % 256 == 0
    if case.geometry:
        assert (B, T, nb) == case.geometry + (1,)  # every lane owns one group
    for call in case.calls(B, T, nb):
        off = case.offsets(call, B, T, nb)
        assert 0 < len(off) <= lane_ref.CAP and len(set(off.tolist())) == len(off) and int(off[-1]) < case.nkeys
        groups = {int(o) // (2 * B) for o in off}
        if call.m is not None:  # the exceptional lane, its neighbours and its thread: first, centre and last key of each
            per = lane_ref.per_thread_of(T)
            assert (walk_ref.centre(call.start >> case.offs, B, T, call.m) + (call.t or 0)) % lane_ref.N == 2 * (call.m + 1) * 2 * B
            for g in [call.m - 1, call.m, call.m + 1] + lane_ref.thread_lanes(T, per, call.m):
                if 0 <= g < T:
                    assert {g * 2 * B, g * 2 * B + B, g * 2 * B + 2 * B - 1} <= set(off.tolist())
        assert {0, T - 1} <= {g % T for g in groups}
        if name in "hi":
            assert nb >= 2 and len(off[off >= 1 << 32]) >= 100
            assert {(1 << 32) - 1, 1 << 32, (1 << 32) + 1, case.nkeys - 1, 0, T * 2 * B, T * 2 * B - 1} <= set(off.tolist())


def test_the_cases_are_the_ones_the_gpu_module_runs():
    count = {name: len(c.calls(*c.plan())) for name, c in lane_ref.CASES.items()}
    assert count == {"a": 12, "b": 4, "c": 3, "d": 2, "e": 1, "f": 1, "g": 2, "h": 1, "i": 1}
    a = lane_ref.CASES["a"]
    nt = (1 << 19) // 8
    assert sorted(c.m for c in a.calls(*a.plan())) == sorted(r * nt + t for r in (0, 3, 4, 7) for t in (0, nt // 2 + 1, nt - 1))
    b = lane_ref.CASES["b"]
    nt = (1 << 18) // 4
    assert sorted(c.m for c in b.calls(*b.plan())) == sorted(r * nt + t for r in (0, 3) for t in (0, nt - 1))
    assert [c.start for c in lane_ref.CASES["c"].calls(*lane_ref.CASES["c"].plan())][:2] == [8, 9]
    assert all(c.start.bit_length() == 200 for k in "cd" for c in lane_ref.CASES[k].calls(*lane_ref.CASES[k].plan()) if c.label.startswith("random"))
    for name, r in (("d", 5), ("e", 6), ("f", 7), ("g", 4)):
        c = lane_ref.CASES[name]
        B, T, nb = c.plan()
        assert c.calls(B, T, nb)[0].m // (T // 8) == r and T >= 1 << 19
    f = lane_ref.CASES["f"]
    B, T, nb = f.plan()
    assert f.calls(B, T, nb)[0].start == (2 * (7 * (T // 8) + 5) + 3) * B
    g1, g2 = lane_ref.CASES["g"].calls(*lane_ref.CASES["g"].plan())
    assert (g1.start - 8 + g1.t) % lane_ref.N == (g1.m + 1) * 16 and g2.t == g1.t + 1 and g2.start == g1.start
    assert lane_ref.CASES["h"].nkeys == lane_ref.CASES["i"].nkeys == (1 << 32) + (1 << 22) + 5 and lane_ref.CASES["i"].cap == 16


@pytest.mark.parametrize("name", list(lane_ref.CASES))
def test_filter_condition_and_two_records_of_every_call(name):
    """the filter of every call holds all of its hashes at a bit density below 0.002, and two expected records per call are the hash (or
    the x) of the oracle's point of that key"""
    case = lane_ref.CASES[name]
    B, T, nb = case.plan()
    for call in case.calls(B, T, nb):
        want = case.expected(call, B, T, nb)
        assert len(want) == len(case.offsets(call, B, T, nb)) and np.array_equal(want["key_offset"], case.offsets(call, B, T, nb))
        words = lane_ref.planted_filter(want["h160"])
        assert len(words) == 1 << 20 and lane_ref.density(words) < 0.002
        assert lane_ref.density(words) * (1 << 26) <= 20 * len(want)
        assert orc.blf_has_many(words, want["h160"]).all()
        picks = [len(want) // 3, len(want) - 1]
        if call.m is not None:  # ... one of them the exceptional lane's centre
            picks[0] = int(np.searchsorted(want["key_offset"], call.m * 2 * B + B))
        for i in picks:
            k = (call.start + (int(want["key_offset"][i]) << case.offs) + (call.t or 0)) % lane_ref.N
            x, y = orc.point_of(k)
            if call.t is None:
                assert [int(w) for w in want["h160"][i]] == orc.hash160(x, y, True) and want["type"][i] == 1, (call.label, i)
            else:
                assert [int(w) for w in want["h160"][i]] == pub_ref.words5(x) and want["type"][i] == 5, (call.label, i)
            assert want["endo"][i] == 0


def test_lanes_that_differ_names_the_lane():
    case = lane_ref.CASES["b"]
    B, T, nb = case.plan()
    call = case.calls(B, T, nb)[1]
    want = case.expected(call, B, T, nb)
    assert lane_ref.lanes_that_differ(want, want, B, T) == []
    lane_keys = (want["key_offset"] // (2 * B)) == call.m
    assert lane_keys.sum() == 3
    assert lane_ref.lanes_that_differ(want[~lane_keys], want, B, T) == [call.m]
    got = want.copy()
    got["h160"][0, 0] ^= 1
    assert lane_ref.lanes_that_differ(got, want, B, T) == [0]
