"""emit33_ypar (csrc/emit33.h) on the GPU: y's parity of a walked point from a partial product, in the addr33-only add kernels.

The function by itself on raw limbs (Device.diag_limbs, op LIMB_PAR33): the operand sets the host program csrc/tools/par33_host.cpp made and
checked (tests/par33_cases.py: 4096 random sets, limbs 5..8 at 0 / the ceiling in every pattern, sets on both sides of the guard, sets on
which the short way alone is wrong) - parity AND path taken must be the host's, and both paths must have run.  Then the two kernels that
use it, k_add<true, false, false> and k_add<true, false, true>, through one all-ones-filter `add` call each at T = 256 (tests/test_gpu_emit33.py
runs them at T = 512): two groups per lane, the last one ragged, a lane's centre on the jump point; every record against the oracle.  And
2^19 keys in one call, so that the kernel's own exact path - out of line, once in 2^16 keys - has run when the hashes are compared."""
import numpy as np
import pytest

import limb_cases
import orc
import par33_cases as C

pytestmark = pytest.mark.gpu
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
LAM = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
B, T = 8, 256
NKEYS = 2 * T * 2 * B - 11  # 512 groups of 16: two per lane on 256 lanes, the last one ragged (5 keys)
START = T * 2 * B - B - 2 * (2 * B)  # lane 2's centre, START + B + 2 * 2B, is the jump point T * 2B * G: the tangent path
END = START + -(-NKEYS // 2048) * 2048  # the oracle hashes whole groups of 2048


def test_parity_and_path_on_raw_limbs():
    from ecloop_amd import Device
    rc, text, recs = C.run(12)  # set 1: 4096 sets, all kept
    assert rc == 0, text[-3000:]
    s = recs["set"]
    assert (s == 1).sum() == 4096 and (s == 2).sum() == 4096 and (s == 3).sum() >= 512 and (s == 4).sum() >= 64
    full = np.zeros((len(recs), limb_cases.LIMB_IN, 9), dtype=np.uint32)
    full[:, 0], full[:, 1], full[:, 2] = recs["lam"], recs["b"], recs["Y"]
    d = Device(0)
    try:
        out, flag = d.diag_limbs(C.LIMB_PAR33, full)
    finally:
        d.close()
    bad = np.nonzero((flag != recs["par"]) | (out[:, 0, 0] != recs["path"]))[0]
    assert not len(bad), (int(bad[0]), recs[bad[0]].tolist(), int(flag[bad[0]]), int(out[bad[0], 0, 0]))
    assert (out[:, 0, 0] == 1).sum() >= 256 + 64 and (out[:, 0, 0] == 0).sum() >= 2 * 4096 + 256  # both paths ran on the device
    assert not out[:, 0, 1:].any() and not out[:, 1:].any()


def oracle_lines(endo):
    rc, out, n, _, hashed = orc.add_range(orc.OrcFilter(bloom_words=ONES), START, END, endo=endo, verify=False, threads=4, cap=1 << 17)
    assert rc == 0 and hashed == END - START
    return orc.found_lines(out, n)


def add_call(endo):
    from ecloop_amd import Device
    d = Device(0, endo=endo)
    try:
        d.set_geometry(B, T)
        d.set_bloom(ONES)
        assert d.plan_geometry(NKEYS) == (B, T, 2)
        recs, n = d.add_range(START, NKEYS, cap=(6 if endo else 1) * NKEYS)
        assert n == len(recs)
        req, cov, _ = d.coverage()
        assert req == cov == NKEYS
        return recs
    finally:
        d.close()


def test_every_key_of_a_ragged_call_at_256_lanes():
    assert START + B + 2 * 2 * B == T * 2 * B
    recs = add_call(False)
    assert all(int(r["compressed"]) == 1 and int(r["endo"]) == 0 for r in recs)
    got = sorted("addr33\t%s\t%064x" % (orc.hex160(r["h160"]), START + int(r["key_offset"])) for r in recs)
    want = sorted(l for l in oracle_lines(False) if START <= int(l.split("\t")[2], 16) < START + NKEYS)
    assert len(want) == NKEYS and got == want


def test_half_a_million_keys_so_that_the_exact_path_of_the_kernel_runs():
    """the guard fires once in 2^16 keys and the kernel then walks the point again out of line (walk_ypar_exact, add_kernel.h), which the
    8 181 keys above most likely never reach: 2^19 keys (8 expected by that way) in the library's own geometry through the all-ones
    filter, the hash160 of every key against the oracle's - a wrong parity is a wrong prefix byte and another hash"""
    from ecloop_amd import Device
    start, n = 0x33000000, 1 << 19
    d = Device(0)
    try:
        d.set_bloom(ONES)
        recs, got = d.add_range(start, n, cap=n)
        assert got == len(recs) == n
    finally:
        d.close()
    rc, out, nout, _, hashed = orc.add_range(orc.OrcFilter(bloom_words=ONES), start, start + n, verify=False, threads=8, cap=n)
    assert rc == 0 and hashed == n and nout == n
    want = np.frombuffer(out, dtype=np.dtype([("h160", "<u4", (5,)), ("compressed", "u1"), ("endo", "u1"), ("pad", "u1", (2,)), ("pk", "<u8", (4,))]))[:n]
    assert not want["pk"][:, 1:].any() and (want["compressed"] == 1).all() and (recs["compressed"] == 1).all()
    want = want[np.argsort(want["pk"][:, 0])]
    recs = recs[np.argsort(recs["key_offset"])]
    assert np.array_equal(want["pk"][:, 0], start + recs["key_offset"])
    bad = np.nonzero((want["h160"] != recs["h160"]).any(axis=1))[0]
    assert not len(bad), (len(bad), hex(start + int(recs["key_offset"][bad[0]])), orc.hex160(recs["h160"][bad[0]]), orc.hex160(want["h160"][bad[0]]))


def test_a_quarter_million_keys_with_the_endomorphism_so_that_its_exact_block_runs():
    """k_add<true, false, true> keeps its exact way in place (add_walk.inc), another body than walk_ypar_exact: 2^18 keys (4 expected by
    that way; a wrong parity there spoils all six images of the key) through the all-ones filter.  The hash160 of every image must be
    one the oracle has for the same keys - the two lists are equal as multisets - and every 61st record is matched to the oracle's record
    of its own private key (calc_priv, main.c:267-276)"""
    from ecloop_amd import Device
    start, n = 0x35000000, 1 << 18
    d = Device(0, endo=True)
    try:
        d.set_bloom(ONES)
        recs, got = d.add_range(start, n, cap=6 * n)
        assert got == len(recs) == 6 * n
    finally:
        d.close()
    rc, out, nout, _, hashed = orc.add_range(orc.OrcFilter(bloom_words=ONES), start, start + n, endo=True, verify=False, threads=8, cap=6 * n)
    assert rc == 0 and hashed == n and nout == 6 * n
    want = np.frombuffer(out, dtype=np.dtype([("h160", "<u4", (5,)), ("compressed", "u1"), ("endo", "u1"), ("pad", "u1", (2,)), ("pk", "<u8", (4,))]))[:nout]
    assert (want["compressed"] == 1).all() and (recs["compressed"] == 1).all()
    # every (key, image) once
    pairs = np.sort(recs["key_offset"] * 8 + recs["endo"])
    assert np.array_equal(pairs, (np.arange(n, dtype=np.uint64)[:, None] * 8 + np.arange(6, dtype=np.uint64)[None, :]).ravel())
    # the same hashes, all of them
    mine = np.sort(np.ascontiguousarray(recs["h160"]).view("V20").ravel())
    theirs = np.sort(np.ascontiguousarray(want["h160"]).view("V20").ravel())
    assert np.array_equal(mine, theirs), int((mine != theirs).sum())
    # ... and each with its own key, on a sample
    order = np.lexsort(tuple(want["pk"][:, j] for j in range(4)))
    keys = want["pk"][order]
    for r in recs[::61]:
        k, e = (start + int(r["key_offset"])) % orc.N, int(r["endo"])
        k = k * pow(LAM, e // 2, orc.N) % orc.N
        k = (-k) % orc.N if e & 1 else k
        w = [(k >> (64 * j)) & orc.MASK64 for j in range(4)]
        lo, hi = 0, len(keys)
        while lo < hi:  # lexsort: the last key is the most significant
            mid = (lo + hi) // 2
            if tuple(int(v) for v in keys[mid][::-1]) < tuple(w[::-1]):
                lo = mid + 1
            else:
                hi = mid
        assert lo < len(keys) and [int(v) for v in keys[lo]] == w and np.array_equal(want["h160"][order[lo]], r["h160"]), (hex(k), e)


def test_every_endomorphism_image_of_a_ragged_call_at_256_lanes():
    recs = add_call(True)
    assert len(recs) == 6 * NKEYS and all(int(r["compressed"]) == 1 for r in recs)

    def priv(off, e):  # calc_priv (main.c:267-276)
        k = (START + off) % orc.N
        k = k * pow(LAM, e // 2, orc.N) % orc.N
        return (-k) % orc.N if e & 1 else k

    assert sorted((int(r["key_offset"]), int(r["endo"])) for r in recs) == [(o, e) for o in range(NKEYS) for e in range(6)]
    got = ["addr33\t%s\t%064x" % (orc.hex160(r["h160"]), priv(int(r["key_offset"]), int(r["endo"]))) for r in recs]
    want = set(oracle_lines(True))  # the oracle's whole groups: a superset of the call's keys
    assert len(want) == 6 * (END - START) and all(l in want for l in got)
