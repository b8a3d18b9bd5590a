"""tests/mul_ref.py, the reference of tests/test_gpu_mul_types.py, on the CPU: its restatement of the call's cutting gives the two shapes
their pieces, rounds and partly filled waves; every planted scalar sits at the (piece, round, thread) it claims; the tables agree, on every
997th scalar and on all planted ones, with paths that share nothing with them (the oracle's double-and-add, the pure-Python sponge,
tr_ref's own addition with pow(), pub_ref, p2sh_ref on hex text, the FakeDevice's verify); and the three-word filter leaves something
to compare in every context."""
import numpy as np
import pytest

import eth_ref
import mul_ref
import orc
import p2sh_ref
import pub_ref
import tr_ref
import walk_ref
from fake_device import FakeDevice
from mul_ref import NA, NB

N = orc.N


def test_geometry_restatement_gives_the_two_shapes():
    assert mul_ref.geometry(196607) == (1, 196608) and mul_ref.geometry(196608) == (1, 196608) and mul_ref.geometry(196609) == (2, 98560)
    assert NA == 262221 and mul_ref.pieces(NA) == [(0, NA, 2, 131328, 0)]  # one piece, two rounds
    assert NA - 131328 - 1 == 130892 and 130892 // 64 == 2045 and 130892 % 64 == 12  # round 1: wave 2045 has lanes 0 ... 12, nothing above
    assert mul_ref.place(NA, 131327) == (0, 0, 131327) and mul_ref.place(NA, 131328) == (0, 1, 0) and mul_ref.place(NA, NA - 1) == (0, 1, 130892)
    # B: one scalar per thread on the context's stream, then three per thread on the second one; the five scalars past the doubled piece go along
    assert NB == 589829 and mul_ref.pieces(NB) == [(0, 196608, 1, 196608, 0), (196608, 393221, 3, 131328, 1)]
    assert mul_ref.place(NB, 196607) == (0, 0, 196607) and mul_ref.place(NB, 196608) == (1, 0, 0)
    assert mul_ref.place(NB, 196608 + 2 * 131328) == (1, 2, 0) and mul_ref.place(NB, NB - 1) == (1, 2, 130564)
    # calls of the sizes the existing mul tests use have one scalar per thread
    assert mul_ref.pieces((1 << 16) + 77) == [(0, (1 << 16) + 77, 1, 65792, 0)]
    # a long call: pieces of 1, 2, 4, 8 and then 10 scalars per resident thread, alternating streams
    assert [(m // 196608, R, s) for _, m, R, _, s in mul_ref.pieces(1 << 24)[:6]] == [(1, 1, 0), (2, 2, 1), (4, 4, 0), (8, 8, 1), (10, 10, 0), (10, 10, 1)]
    assert sum(m for _, m, _, _, _ in mul_ref.pieces(1 << 24)) == 1 << 24


def test_every_planted_scalar_sits_where_it_claims():
    K, planted = mul_ref.scalars()
    assert len(K) == NB and len({p[6] for p in planted}) == len(planted)
    kinds = {}
    for shape, piece, rnd, thread, kind, value, i in planted:
        assert mul_ref.place(mul_ref.SHAPE_N[shape], i) == (piece, rnd, thread), (shape, kind)
        assert mul_ref.ints_of(K[i:i + 1]) == [value]
        assert (i < NA) == (shape == "A")
        kinds.setdefault((shape, piece, rnd), set()).add(kind.split(",")[0].split(" ")[0])
    # each kind in both rounds of shape A and in the three rounds of B's second piece
    assert sorted(kinds) == [("A", 0, 0), ("A", 0, 1), ("B", 1, 0), ("B", 1, 1), ("B", 1, 2)]
    assert all(k == {"inf", "digit", "short", "bit", "around"} for k in kinds.values())
    at = {(s, p, r, t): v for s, p, r, t, kind, v, _ in planted}
    inf = lambda *where: at.get(where, 1) % N == 0
    for (shape, piece, rnd), wave in mul_ref.WAVES.items():
        t = 64 * wave
        rounds = range(2 if shape == "A" else 3)
        assert inf(shape, piece, rnd, t) and inf(shape, piece, rnd, t + 63) and not any(inf(shape, piece, rnd, t + l) for l in range(1, 63))
        assert all(inf(shape, piece, rnd, t + 64 + l) for l in range(64))  # a whole wave without a point in this round ...
        assert not any(inf(shape, piece, r, t + 64 + l) for l in range(64) for r in rounds if r != rnd)  # ... and with one in the others
        assert [inf(shape, piece, r, t + 128 + 5) for r in rounds] == [r == rnd for r in rounds]  # one round only of a thread (B: the middle one too)
        long = [l for l in range(64) if at[shape, piece, rnd, t + 6 * 64 + l] >= 1 << 40]
        assert long == [17] and at[shape, piece, rnd, t + 6 * 64 + 17] >> 250 == 1
        assert [at[shape, piece, rnd, t + 7 * 64 + l].bit_length() for l in range(64)] == list(range(1, 65))
        assert [at[shape, piece, rnd, t + 8 * 64 + l] for l in range(7)] == [N - 1, N + 1, N + 12345, 2 * N - (1 << 256), (1 << 256) - 1, 1, 2]
        for W in (22, 26):
            mine = [v for s, p, r, _, kind, v, _ in planted if (s, p, r) == (shape, piece, rnd) and kind == "digit edge W=%d" % W]
            assert mine == mul_ref.digit_edge_specials(W)
    assert all(inf("A", 0, r, 300 * 64 + 7) for r in range(2)) and all(inf("B", 1, r, 1400 * 64 + 7) for r in range(3))  # every round of a thread
    # threads whose last round holds no scalar, and the last live lane of the last round's partly filled wave
    assert 131000 > 130892 and inf("A", 0, 0, 131000)
    assert 131000 > 130564 and inf("B", 1, 0, 131000) and inf("B", 1, 1, 131001) and inf("B", 1, 0, 131002) and inf("B", 1, 1, 131002)
    assert inf("A", 0, 1, 130892) and inf("B", 1, 2, 130564)
    # the digit-edge scalars of the existing mul tests are the same helper's
    E = mul_ref.digit_edge_scalars(np.random.default_rng(1), 200, 22)
    assert mul_ref.ints_of(E[:len(mul_ref.digit_edge_specials(22))]) == mul_ref.digit_edge_specials(22)


def sample():
    K, planted = mul_ref.scalars()
    return sorted(set(range(0, NB, 997)) | {p[6] for p in planted})


def test_ok_is_zero_exactly_at_the_scalars_without_a_point():
    K, planted = mul_ref.scalars()
    r = mul_ref.ref()
    ks = mul_ref.ints_of(K)
    none = {i for i, k in enumerate(ks) if k % N == 0}
    assert none == {p[6] for p in planted if p[5] % N == 0} and len(none) == 352
    assert set(np.nonzero(~r.ok)[0].tolist()) == none
    for table in ("h33", "h65", "p2sh", "eth", "pub", "tr"):
        assert not getattr(r, table)[sorted(none)].any(), table


def test_tables_agree_with_independent_paths_on_the_sample():
    K, _ = mul_ref.scalars()
    r = mul_ref.ref()
    idx = [i for i in sample() if r.ok[i]]
    ks = mul_ref.ints_of(K[idx])
    pts = [orc.point_of(k % N) for k in ks]  # double-and-add, not the table
    xs, ys = mul_ref.ints_of(r.points[0][idx]), mul_ref.ints_of(r.points[1][idx])
    assert list(zip(xs, ys)) == pts
    h33, h65, ok = FakeDevice().verify([k % N for k in ks])  # (orc.point_of + orc.hash160, one key at a time)
    assert ok.all() and np.array_equal(h33, r.h33[idx]) and np.array_equal(h65, r.h65[idx])
    for j, i in enumerate(idx):
        x, y = pts[j]
        assert eth_ref.eth_words(x, y) == r.eth[i].tolist(), i
        assert tr_ref.words5(tr_ref.output_key(ks[j])) == r.tr[i].tolist(), i
        assert pub_ref.h160_of(ks[j]) == tuple(r.pub[i].tolist()), i
        assert p2sh_ref.p2sh_hex(orc.hex160(h33[j])) == orc.hex160(r.p2sh[i]), i


def test_records_are_one_per_type_and_scalar_with_a_point():
    r = mul_ref.ref()
    live = np.nonzero(r.ok[:NA])[0]
    for name, (letters, _) in mul_ref.CONTEXTS.items():
        recs = r.records(name, 0, NA)
        assert len(recs) == len(letters) * len(live) and not recs["endo"].any()
        for t in letters:
            part = recs[recs["type"] == mul_ref.TYPE[t]]
            assert np.array_equal(part["key_offset"], live.astype(np.uint64)) and np.array_equal(part["h160"], getattr(r, mul_ref.TABLE[t])[live])
    assert mul_ref.TYPE == {"u": 0, "c": 1, "s": 2, "e": 3, "t": 4, "x": 5}
    # a later part of the array as a call of its own: key_offset counts from the call's first scalar
    part, whole = r.records("cus", 1000, 5000), r.records("cus")
    sel = whole[(whole["key_offset"] >= 1000) & (whole["key_offset"] < 6000)]
    sel["key_offset"] -= 1000
    assert walk_ref.difference(part, sel) == ""


@pytest.mark.parametrize("name", list(mul_ref.CONTEXTS))
def test_three_word_filter_expectation_is_not_empty(name):
    """a condition on the inputs of the GPU test: the filter lets some record of every selected type through, and not all of them; what it
    lets through is what the oracle's single-hash test lets through"""
    from synth import synth_bloom_words
    assert len(mul_ref.CONTEXTS) == 10
    r = mul_ref.ref()
    want, every = r.records(name, 0, NA, mul_ref.FILTER3), r.records(name, 0, NA)
    assert 0 < len(want) < len(every) // 20
    flt = orc.OrcFilter(bloom_words=synth_bloom_words(*mul_ref.FILTER3))
    for t in mul_ref.CONTEXTS[name][0]:
        assert (want["type"] == mul_ref.TYPE[t]).sum() > 100, t
    passing = {(int(a["key_offset"]), int(a["type"])) for a in want}
    for a in every[::257]:
        assert flt.check(a["h160"].tolist()) == ((int(a["key_offset"]), int(a["type"])) in passing)
    rounds = {mul_ref.place(NA, int(i))[1] for i in want["key_offset"]}
    assert rounds == {0, 1}  # records from both rounds
