"""The addr33-only emit path of the add kernels (csrc/emit33.h, k_add<true, false, ENDO>) on the GPU, every result against the oracle:
the function by itself on raw limbs at the magnitude ceilings (Device.diag_limbs, the operand sets the CPU test feeds the host build),
and the kernel through small `add` calls in which every path of the filter test runs - an all-ones filter (every key is parked,
recorded and compared), a 3-word filter (bloom_mod with a word count that is no power of two) and a 2^16-word one (the ring stages thin
the candidates out)."""
import numpy as np
import pytest

import emit33_cases
import limb_cases
import orc
from synth import synth_bloom_words

pytestmark = pytest.mark.gpu
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
LAM = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
B, T = 8, 512
NKEYS = 3 * (1 << 12) + 5  # 769 groups of 16: two per lane on 512 lanes, the last one ragged
START = T * 2 * B - B - 2 * (2 * B)  # lane 2's centre, START + B + 2 * 2B, is the jump point T * 2B * G: the tangent path


def test_emit33_raw_limbs_on_the_device():
    from ecloop_amd import Device
    cases = emit33_cases.operand_sets()
    full = np.zeros((len(cases), limb_cases.LIMB_IN, 9), dtype=np.uint32)
    full[:, :2] = cases
    d = Device(0)
    try:
        out, flag = d.diag_limbs(limb_cases.OP["LIMB_EMIT33"], full)
    finally:
        d.close()
    want = emit33_cases.reference()
    got = np.concatenate([out[:, 1, :5], flag[:, None], out[:, 1, 5:7]], axis=1)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), (int(bad[0]), cases[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())
    assert not out[:, 2:].any() and not out[:, 1, 7:].any()
    # the message words: prefix byte 2 | parity, then x mod p big-endian, then the pad byte
    xs = limb_cases.values(cases[:, 0]) % limb_cases.P
    for i in range(0, len(cases), 7):
        m = ((2 | int(want[i, 5])) << 256 | int(xs[i])) << 24 | 0x800000
        assert [int(w) for w in out[i, 0]] == [(m >> (32 * (8 - j))) & 0xFFFFFFFF for j in range(9)], i


def oracle_lines(words, endo=False):
    """the oracle's found lines over the reference's whole groups that cover the call (it hashes 2048 keys at a time)"""
    end = START + -(-NKEYS // 2048) * 2048
    rc, out, n, _, hashed = orc.add_range(orc.OrcFilter(bloom_words=words), START, end, endo=endo, verify=False, threads=4, cap=1 << 17)
    assert rc == 0 and hashed == end - START
    return orc.found_lines(out, n)


def of_the_call(lines):
    return sorted(l for l in lines if START <= int(l.split("\t")[2], 16) < START + NKEYS)


@pytest.fixture(scope="module")
def walked_keys():
    """hash160 of every key of the call by the oracle, once"""
    lines = of_the_call(oracle_lines(ONES))
    assert len(lines) == NKEYS
    return lines


def lines_of(recs, endo=False):
    assert all(int(r["compressed"]) == 1 and (endo or int(r["endo"]) == 0) for r in recs)
    return sorted("addr33\t%s\t%064x" % (orc.hex160(r["h160"]), START + int(r["key_offset"])) for r in recs)


def add_call(words, cap):
    from ecloop_amd import Device
    d = Device(0)
    try:
        d.set_geometry(B, T)
        d.set_bloom(words)
        assert d.plan_geometry(NKEYS) == (B, T, 2)
        recs, n = d.add_range(START, NKEYS, cap=cap)
        assert n == len(recs)
        req, cov, _ = d.coverage()
        assert req == cov == NKEYS
        return recs
    finally:
        d.close()


def test_every_key_of_a_ragged_call_through_the_all_ones_filter(walked_keys):
    assert (START + B + 2 * 2 * B) == T * 2 * B
    assert lines_of(add_call(ONES, NKEYS)) == walked_keys


@pytest.mark.parametrize("nwords,mode", [(3, "a|b"), (1 << 16, "a&(b|c)")])
def test_found_lists_through_real_filters(nwords, mode):
    words = synth_bloom_words(nwords, 33, mode)
    want = of_the_call(oracle_lines(words))
    assert lines_of(add_call(words, NKEYS)) == want
    if nwords == 3:
        assert len(want) > 0  # three words at density 0.75: keys pass all twenty probes, so the rings' later stages ran

def test_endomorphism_images_through_the_all_ones_filter():
    """k_add<true, false, true>: the six images of every key of a ragged call (beta x and beta^2 x through the same message words, the
    prefix byte flipped for -y), each against the oracle's record for it"""
    from ecloop_amd import Device
    nkeys = 2048 + 5
    d = Device(0, endo=True)
    try:
        d.set_geometry(B, 256)
        d.set_bloom(ONES)
        recs, n = d.add_range(START, nkeys, cap=6 * nkeys)
        assert n == len(recs) == 6 * nkeys
    finally:
        d.close()

    def priv(off, e):  # calc_priv (main.c:267-276)
        k = (START + off) % orc.N
        k = k * pow(LAM, e // 2, orc.N) % orc.N
        return (-k) % orc.N if e & 1 else k

    assert sorted((int(r["key_offset"]), int(r["endo"])) for r in recs) == [(o, e) for o in range(nkeys) for e in range(6)]
    got = ["addr33\t%s\t%064x" % (orc.hex160(r["h160"]), priv(int(r["key_offset"]), int(r["endo"]))) for r in recs]
    want = set(oracle_lines(ONES, endo=True))  # the oracle's whole groups: a superset of the call's keys
    assert len(want) == 6 * (-(-NKEYS // 2048) * 2048) and all(l in want for l in got)
