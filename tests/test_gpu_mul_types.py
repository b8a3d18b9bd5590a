"""Every `mul` kernel scalar by scalar: csrc/mul_check.inc - the window sum and its out-of-line complete sum, a thread's product chain with
one inversion, the backward pass, the candidate rings - is compiled separately into nine kernels with a register allocation each
(k_mul_check c / u / cu, k_mul_check_p2sh s / cs / us / cus, k_mul_check_eth, k_mul_points_tr followed by k_tr_check, k_mul_check_pub).

Ten contexts (`c` and `cu` are the controls: tests/test_gpu_add.py checks them scalar by scalar already, so a failure there points at this
test), each on one Device through the scalars of tests/mul_ref.py:

  A  2^18 + 77 scalars at the automatic width (22 bits): one piece, two scalars per thread, the second round ending inside a wave - with
     the all-ones filter, then through the three-word filter of bit density 0.75 of tests/test_gpu_walk_steps.py (the rings' later stages
     over two rounds with dead lanes; Taproot: k_tr_check's probe stage; public keys: cand1_flush<5, true>).
  B  196 608 + 393 216 + 5 scalars on the 26-bit table: a piece of one scalar per thread on the context's stream, then a piece of three per
     thread on the second compute stream with its own parking space, whose key offsets start at 196 608.

Planted in both rounds of A and in the three rounds of B's second piece: 0 and n (in one round only of a thread, in every round of a thread,
in a thread whose later round is empty, in the last live lane, in lanes 0 and 63, in a whole wave), the digit-edge scalars of the 22- and
the 26-bit table, a wave of short scalars with one long one, bit lengths 1 ... 64, the scalars around n.  tests/test_mul_ref.py asserts on
the CPU where each one sits.  The records must equal mul_ref.MulRef.records() exactly, each once, the total their number, and the three
coverage totals must grow by the call's scalars (those without a point are counted, not reported).  Every assertion is an equality.

And shape A again on every context at 8 and at 13 bits (ecl_hip_set_mul_window): at 22 and 26 bits only the planted scalars take the
out-of-line complete sum, at 8 bits every eighth random scalar has a zero signed digit and the call is mixed into nearly every thread's
chain - in both rounds of a thread, in the first alone, in the second alone (tests/test_digit_ref.py counts 1820, 13 690 and 13 412 such
threads; on context `t` k_tr_check meets the same on the tweaks' digits: 1730, 13 468, 13 330).  The expectation does not depend on the width.

Then the calls that produce more records than fit: the header's words for `mul` (ECL_E_OVERFLOW, ecl_hip_fetch_found, the repeat with
cap = total), and engine.KeySearch.cmd_mul on a context with three records per scalar."""
import ctypes as C
import time

import numpy as np
import pytest

import mul_ref
from mul_ref import CONTEXTS, FILTER3, NA, NB, ONES, canon, difference
from synth import synth_bloom_words

pytestmark = pytest.mark.gpu


def mul_call(d, K, cap):
    """ecl_hip_mul_batch on the array as it is -> (return code, records, total)"""
    from ecloop_amd import capi
    K = np.ascontiguousarray(K, dtype=np.uint64)
    out = np.zeros(cap, dtype=capi.FOUND_DTYPE)
    cnt = C.c_uint32()
    rc = d.lib.ecl_hip_mul_batch(d.h, K.ctypes.data, len(K), out.ctypes.data, cap, C.byref(cnt))
    return rc, out[: min(cnt.value, cap)], cnt.value


def checked_call(d, name, K, want, what, wrong):
    """mul_batch over K: the records are the reference's, each once; the total is their number; the coverage totals grow by the call's
    scalars.  What is not so goes to `wrong`, so that a failing context names every shape that fails"""
    before, ms, t0 = d.coverage(), d.mul_timing()[0], time.perf_counter()
    rc, recs, total = mul_call(d, K, len(want) + 16)
    t1 = time.perf_counter()
    grown = tuple(b - a for a, b in zip(before, d.coverage()))
    print("%s %s: rc %d, %d records, %d expected, coverage +%s; device %.2f ms, call %.0f ms" % (name, what, rc, total, len(want), grown, d.mul_timing()[0] - ms, 1e3 * (t1 - t0)))
    if rc != 0:
        wrong.append("%s: return code %d (%s)" % (what, rc, d.lib.ecl_hip_last_error(d.h).decode()))
    if not total == len(recs) == len(want):
        wrong.append("%s: a total of %d, %d records, %d expected" % (what, total, len(recs), len(want)))
    if difference(canon(recs), want) != "":
        wrong.append("%s: %s" % (what, difference(canon(recs), want)))
    if grown != (len(K), len(K), len(K)):
        wrong.append("%s: coverage grew by %s for %d scalars" % (what, grown, len(K)))


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_every_scalar_of_every_round_and_piece(name):
    from ecloop_amd import Device
    K, _ = mul_ref.scalars()
    ref = mul_ref.ref()
    letters, kw = CONTEXTS[name]
    live_a, live_b = int(ref.ok[:NA].sum()), int(ref.ok.sum())
    want_a, want_f, want_b = ref.records(name, 0, NA), ref.records(name, 0, NA, FILTER3), ref.records(name)
    assert len(want_a) == len(letters) * live_a and len(want_b) == len(letters) * live_b and 0 < len(want_f) < len(want_a)  # (the expectation)
    wrong = []
    t0 = time.perf_counter()
    d = Device(0, **kw)
    try:
        d.set_bloom(ONES)
        checked_call(d, name, K[:NA], want_a, "A", wrong)
        assert d.mul_window() == 22
        d.set_bloom(synth_bloom_words(*FILTER3))
        checked_call(d, name, K[:NA], want_f, "A, three-word filter", wrong)
        d.set_bloom(ONES)
        d.set_mul_window(26)
        checked_call(d, name, K, want_b, "B, 26-bit table", wrong)
        assert d.mul_window() == 26
    finally:
        d.close()
    print("%s: %.1f s with the context's bring-up and both tables" % (name, time.perf_counter() - t0))
    assert wrong == [], "%s: %s" % (name, "; ".join(wrong))


@pytest.mark.parametrize("W", [8, 13])
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_every_kernel_at_narrow_widths(name, W):
    from ecloop_amd import Device
    K, _ = mul_ref.scalars()
    ref = mul_ref.ref()
    letters, kw = CONTEXTS[name]
    want_a = ref.records(name, 0, NA)
    assert len(want_a) == len(letters) * int(ref.ok[:NA].sum())  # (the expectation)
    assert mul_ref.pieces(NA) == [(0, NA, 2, 131328, 0)]  # one piece, two scalars per thread
    wrong = []
    d = Device(0, **kw)
    try:
        d.set_bloom(ONES)
        d.set_mul_window(W)
        checked_call(d, name, K[:NA], want_a, "A, W = %d" % W, wrong)
        assert d.mul_window() == W
    finally:
        d.close()
    assert wrong == [], "%s: %s" % (name, "; ".join(wrong))


# ---------------------------------------------------------------------------------------------- calls past the record cap
OVER_N = (1 << 19) + 8  # scalars of a `cu` call that produces more records than the device keeps (2^20)


def test_overflow_fetch_and_repeat_as_the_header_says():
    """include/ecloop_hip.h for a mul call with more records than `cap`: ECL_E_OVERFLOW with *nout = the total; the device has kept
    max(cap, 2^20) records, ecl_hip_fetch_found hands out those behind the first `cap` and says so when there were more; the call
    repeated with cap = total delivers them all"""
    from ecloop_amd import Device, capi
    ref = mul_ref.plain_ref(OVER_N, 606)
    want = ref.records("cu")
    assert len(want) == 2 * OVER_N == (1 << 20) + 16
    d = Device(0, a33=True, a65=True)
    try:
        d.set_bloom(ONES)
        rc, first, total = mul_call(d, ref.K, 100)
        assert rc == capi.E_OVERFLOW and total == (1 << 20) + 16 and len(first) == 100
        rest = d.fetch_found(100, total - 100)
        assert len(rest) == (1 << 20) - 100  # what the device kept, not what the call produced: the caller has to repeat
        got = canon(np.concatenate([first, rest]))
        slot = 2 * got["key_offset"].astype(np.int64) + got["type"]  # `want` holds (offset, addr65), (offset, addr33) for every offset in turn
        assert len(np.unique(slot)) == len(slot) == 1 << 20 and np.array_equal(got, want[slot])  # distinct members of the expectation
        rc, recs, total2 = mul_call(d, ref.K, total)
        assert rc == 0 and total2 == total == len(recs) and difference(canon(recs), want) == ""
    finally:
        d.close()


def test_engine_cmd_mul_keeps_every_record_of_a_dense_filter():
    """KeySearch.cmd_mul on a context with three records per scalar through the all-ones filter: a chunk of 2^16 scalars produces
    3 * 2^16 records, more than the 2 * 2^16 the chunk's buffer holds - the rest is fetched (engine.add_keys' loop), none is dropped"""
    from ecloop_amd.engine import Filter, KeySearch
    n = 1 << 16
    ref = mul_ref.MulRef(mul_ref.plain_ref(OVER_N, 606).K[:n])
    ks = mul_ref.ints_of(ref.K)
    s = KeySearch(Filter(ONES), device=0, a33=True, a65=True, p2sh=True)
    try:
        found = s.cmd_mul(ks)
        got = sorted((r.label, tuple(r.h160), r.pk) for r in found)
        assert s.k_found == len(found) and s.k_checked == n
    finally:
        s.close()
    want = sorted((label, tuple(h), k) for label, table in (("addr33", ref.h33), ("addr65", ref.h65), ("p2sh", ref.p2sh)) for h, k in zip(table.tolist(), ks))
    assert len(got) == 3 * n and got == want
