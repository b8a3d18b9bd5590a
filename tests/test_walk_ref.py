"""tests/walk_ref.py, the reference of tests/test_gpu_walk_steps.py, on the CPU: its addr33 / addr65 expectations against the oracle-backed
FakeDevice on the same calls, its P2SH / Ethereum / Taproot tables against the known answers of those types' own tests, the starts of
the shapes against the walk's arithmetic, and the three-word filter leaving something to compare in every context."""
import numpy as np
import pytest

import orc
import walk_ref
from fake_device import FakeDevice


@pytest.mark.parametrize("shape", list(walk_ref.SHAPES))
def test_starts_put_lane_2_on_the_jump_point_and_the_tail_in_round_four(shape):
    B, T, start, nkeys = walk_ref.SHAPES[shape]
    sweep = T * 2 * B  # the keys of one round, and the scalar of the jump point J = T * 2B * G
    assert walk_ref.centre(start, B, T, 2) == sweep
    assert [walk_ref.centre(start, B, T, g) for g in range(T)].count(sweep) == 1  # that lane alone
    assert -(-nkeys // sweep) == 4 and 0 < nkeys - 3 * sweep < 2 * B  # four rounds; the fourth: part of lane 0's group, nothing else
    # the lane's later centres are what the tangent leads to: 2 C, 3 C, 4 C
    assert [walk_ref.centre(start, B, T, 2, r) for r in range(4)] == [sweep * (r + 1) for r in range(4)]
    # shape C: a whole sweep, then a call that resumes it - the tangent's centre is what the first call leaves behind for lane 2
    if shape == "A":
        assert walk_ref.centre(start + sweep, B, T, 2) == 2 * sweep and start + sweep + sweep + 5 <= start + nkeys


@pytest.mark.parametrize("shape", list(walk_ref.SHAPES))
@pytest.mark.parametrize("name", ["c", "u", "cu", "c-endo", "u-endo", "cu-endo"])
def test_addr33_and_addr65_expectations_equal_the_fake_device(name, shape):
    _, _, start, nkeys = walk_ref.SHAPES[shape]
    letters, endo, kw = walk_ref.CONTEXTS[name]
    want = walk_ref.ref_of(shape).records(name)
    assert len(want) == nkeys * len(letters) * (6 if endo else 1)
    d = FakeDevice(0, a33=kw["a33"], a65=kw["a65"], endo=endo)
    d.set_bloom(walk_ref.ONES)
    recs, n = d.add_range(start, nkeys, cap=len(want) + 16)
    assert n == len(recs) and walk_ref.difference(walk_ref.canon(recs), want) == ""
    if shape == "A" and name in ("cu", "c-endo"):  # ... and a later part of the range as a call of its own (shape C's second call)
        recs, n = d.add_range(start + 4096, 4101, cap=4101 * 12 + 16)
        assert n == len(recs) and walk_ref.difference(walk_ref.canon(recs), walk_ref.ref_of(shape).records(name, 4096, 4101)) == ""


def test_canon_and_difference_tell_records_apart():
    want = walk_ref.ref_of("B").records("cu")
    assert walk_ref.difference(walk_ref.canon(want[::-1]), want) == ""
    for spoil in ("h160", "endo", "type", "key_offset"):
        got = want.copy()
        got[spoil][777] ^= 1
        assert walk_ref.difference(walk_ref.canon(got), want) != "", spoil
    assert walk_ref.difference(want[:-1], want) != "" and walk_ref.difference(walk_ref.canon(np.concatenate([want, want[5:6]])), want) != ""


def test_p2sh_eth_and_taproot_tables_hold_the_known_answers():
    import test_gpu_eth
    import test_gpu_p2sh
    import test_gpu_tr
    import tr_ref
    for k, h in test_gpu_p2sh.KNOWN.items():
        r = walk_ref.WalkRef(k, 1)
        assert orc.hex160(r.p2sh[0, 0]) == h and orc.hex160(r.records("s")["h160"][0]) == h, hex(k)
        assert [int(w) for w in r.h33[0, 0]] == test_gpu_p2sh.h33_of(k)
    for k, h in test_gpu_eth.KNOWN.items():
        r = walk_ref.WalkRef(k, 1)
        assert orc.hex160(r.eth[0, 0]) == h and orc.hex160(r.records("e-endo")["h160"][0]) == h, hex(k)
    for k, q in test_gpu_tr.KNOWN.items():
        r = walk_ref.WalkRef(k, 1)
        assert list(r.tr[0, 0]) == tr_ref.words5(q) and [int(w) for w in r.records("t")["h160"][0]] == tr_ref.words5(q), hex(k)
    r = walk_ref.WalkRef(1, 2)  # two keys of one table: offset 1 is key 2
    assert orc.hex160(r.p2sh[1, 0]) == test_gpu_p2sh.KNOWN[2] and orc.hex160(r.eth[1, 0]) == test_gpu_eth.KNOWN[2]
    assert list(r.tr[1, 0]) == tr_ref.words5(test_gpu_tr.KNOWN[2])
    types = walk_ref.ref_of("B").records("cus-endo")  # the type codes and the image numbers of a context with everything
    assert sorted(set(types["type"].tolist())) == [0, 1, 2] and sorted(set(types["endo"].tolist())) == list(range(6))
    assert set(walk_ref.ref_of("B").records("e")["type"].tolist()) == {3} and set(walk_ref.ref_of("B").records("t")["type"].tolist()) == {4}


@pytest.mark.parametrize("name", list(walk_ref.CONTEXTS))
def test_three_word_filter_expectation_is_not_empty(name):
    """a condition on the inputs of the GPU test: the filter lets some record of every context through, and not all of them; and what it
    lets through is what the oracle's own filtered walk reports (addr33 / addr65: the FakeDevice with that filter)"""
    from synth import synth_bloom_words
    assert len(walk_ref.CONTEXTS) == 17
    _, _, start, nkeys = walk_ref.SHAPES["A"]
    ref = walk_ref.ref_of("A")
    want, every = ref.records(name, filter3=walk_ref.FILTER3), ref.records(name)
    assert 0 < len(want) < len(every) // 20
    letters, endo, kw = walk_ref.CONTEXTS[name]
    for t in letters:
        assert (want["type"] == walk_ref.TYPE[t]).any(), t  # of every selected type
    if name in ("c", "cu-endo"):
        d = FakeDevice(0, a33=kw["a33"], a65=kw["a65"], endo=endo)
        d.set_bloom(synth_bloom_words(*walk_ref.FILTER3))
        recs, n = d.add_range(start, nkeys, cap=1 << 16)
        assert n == len(recs) and walk_ref.difference(walk_ref.canon(recs), want) == ""
