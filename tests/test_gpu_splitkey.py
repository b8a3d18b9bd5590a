"""The split-key vanity search (ECL_PREFIX | ECL_ORIGIN, `-p` with `-k`) on the GPU.

No new reference: with O = k_Q G for a k_Q the test knows, walking O + (a + j) G is walking the keys k_Q + a + j, so the records of an origin
call over [a, a + n) must equal, field for field, those of the plain prefix context over [k_Q + a, k_Q + a + n) with the same table, and both
must equal the oracle's hashes of those keys (tests/orc.py; Ethereum: tests/eth_ref.py) filtered by tests/prefix_ref.py's membership.  The
tables are built as tests/test_gpu_prefix.py builds them (its table_around), around oracle hashes.

Ethereum at n = 2^17 + 3 with -endo is 786 450 Keccak-256 digests, minutes in eth_ref's pure Python: eth_ref.keccak_many is the same sponge
written over numpy arrays, and eth_ref's pure-Python one stays the reference - every record the oracle set keeps (every expected hit) and a fixed
sample of the others are recomputed with eth_ref.eth_words and compared.

Every GPU-using subprocess runs under its own time limit."""
import ctypes as C
import functools
import random
import subprocess

import numpy as np
import pytest

import eth_ref
import orc
import prefix_ref as R
from eth_ref import keccak_many
from support import cli, run_cli
from test_gpu_prefix import keys_of, table_around, table_of

pytestmark = pytest.mark.gpu
P, N = orc.P, orc.N
KQ = 0x3B6F1D9A2C4E8071_95D3A7F20B1C6E48_D27A90C3F15B8E64_0A7C3E912D5F8B46  # the requester's key; Q = KQ G is all the searcher sees
A = 0x9000000001  # the searcher's start scalar
SHAPES = {"5000": 5000, "2^17+3": (1 << 17) + 3}
TYPES = {"c": dict(a33=True), "cu-endo": dict(a33=True, a65=True, endo=True), "e": dict(a33=False, eth=True), "e-endo": dict(a33=False, eth=True, endo=True)}
WHOLE = np.array([R.words5(0) + R.words5(R.TOP)], np.uint32)


@functools.lru_cache(maxsize=None)
def Q():
    return orc.point_of(KQ)


def image_point(pt, e):
    from ecloop_amd.engine import splitkey_image_origin
    return splitkey_image_origin(pt, e)


# ---- the oracle's records of the keys K, K + 1, ... (K = KQ + A): numpy arrays off, words (n, 5), endo, type

def scalars_le(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), np.uint64).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def btc_records(n, endo):
    """hash160 of both serialisations of every key (and, endo: of the keys calc_priv maps it to), by the oracle's mul path"""
    from ecloop_amd.engine import LAMBDA
    K = (KQ + A) % N
    base = [K + j for j in range(n)]
    assert base[-1] < N
    per = [base]
    if endo:
        l1, l2 = [k * LAMBDA % N for k in base], None
        l2 = [k * LAMBDA % N for k in l1]
        per = [base, [N - k for k in base], l1, [N - k for k in l1], l2, [N - k for k in l2]]
    offs, words, endos, types = [], [], [], []
    for e, ks in enumerate(per):
        h33, h65, ok = orc.mul_hash160_many(scalars_le(ks), True, True)
        assert ok.all()
        for comp, h in ((1, h33), (0, h65)):
            offs.append(np.arange(n, dtype=np.uint64)), words.append(h), endos.append(np.full(n, e, np.uint8)), types.append(np.full(n, comp, np.uint8))
    return np.concatenate(offs), np.concatenate(words), np.concatenate(endos), np.concatenate(types)


def consecutive_points(k0, n):
    """the affine points k0 G, (k0 + 1) G, ...: the oracle's point at the head of every block of 1025, the rest by the chord rule with one
    shared inversion per block (Python integers)"""
    B = 1024
    g = orc.point_of(1)
    tab = [g]
    for i in range(2, B + 1):  # i G, i = 1 ... B
        tab.append(orc.point_of(i))
    out, base = [], k0
    while len(out) < n:
        bx, by = orc.point_of(base)
        out.append((bx, by))
        m = min(B, n - len(out))
        dx = [(tab[i][0] - bx) % P for i in range(m)]
        pre = [1] * (m + 1)
        for i in range(m):
            pre[i + 1] = pre[i] * dx[i] % P
        inv = pow(pre[m], -1, P)
        res = [None] * m
        for i in range(m - 1, -1, -1):
            di = inv * pre[i] % P
            inv = inv * dx[i] % P
            lam = (tab[i][1] - by) * di % P
            x3 = (lam * lam - bx - tab[i][0]) % P
            res[i] = (x3, (lam * (bx - x3) - by) % P)
        out.extend(res)
        base += m + 1
    return out


@functools.lru_cache(maxsize=None)
def eth_points(n):
    return consecutive_points((KQ + A) % N, n)


@functools.lru_cache(maxsize=None)
def eth_records(n, endo):
    from ecloop_amd.engine import SPLITKEY_BETA
    pts = eth_points(n)
    b2 = SPLITKEY_BETA * SPLITKEY_BETA % P
    parts, offs, endos = [], [], []
    for e in range(6 if endo else 1):
        m = (1, SPLITKEY_BETA, b2)[e // 2]
        parts.append(b"".join((x * m % P).to_bytes(32, "big") + ((P - y) if e & 1 else y).to_bytes(32, "big") for x, y in pts))
        offs.append(np.arange(n, dtype=np.uint64)), endos.append(np.full(n, e, np.uint8))
    msgs = np.frombuffer(b"".join(parts), np.uint8).reshape(-1, 64)
    words = np.ascontiguousarray(keccak_many(msgs)[:, 12:]).view(">u4").astype(np.uint32).reshape(-1, 5)
    offs, endos = np.concatenate(offs), np.concatenate(endos)
    # eth_ref is the reference: a fixed sample of the records by its own sponge over the oracle's points (the expected hits: oracle_set)
    for i in random.Random("eth sample").sample(range(len(words)), 48):
        assert eth_by_reference(int(offs[i]), int(endos[i])) == [int(w) for w in words[i]]
    return offs, words, endos, np.full(len(words), 3, np.uint8)


def eth_by_reference(off, e):
    return eth_ref.eth_words(*image_point(orc.point_of((KQ + A + off) % N), e))


def records_of(name, n):
    t = TYPES[name]
    if t.get("eth"):
        offs, words, endos, types = eth_records(n, bool(t.get("endo")))
    else:
        offs, words, endos, types = btc_records(n, bool(t.get("endo")))
        keep = np.ones(len(offs), bool)
        if not t.get("a65"):
            keep &= types == 1
        if not t.get("a33"):
            keep &= types == 0
        offs, words, endos, types = offs[keep], words[keep], endos[keep], types[keep]
    return offs, words, endos, types


def tuples_of(offs, words, endos, types, idx):
    return [(int(offs[i]), tuple(int(w) for w in words[i]), int(endos[i]), int(types[i])) for i in idx]


def member_indices(pairs, words):
    """indices of the values inside a range: a conservative cut on the leading 64 bits with numpy, then prefix_ref's membership, exactly"""
    top = (words[:, 0].astype(np.uint64) << np.uint64(32)) | words[:, 1].astype(np.uint64)
    iv = []
    for lo, hi in sorted((lo >> 96, hi >> 96) for lo, hi in pairs):
        if iv and lo <= iv[-1][1]:
            iv[-1][1] = max(iv[-1][1], hi)
        else:
            iv.append([lo, hi])
    los, his = np.array([i[0] for i in iv], np.uint64), np.array([i[1] for i in iv], np.uint64)
    j = np.searchsorted(los, top, "right").astype(np.int64) - 1
    cand = np.nonzero((j >= 0) & (top <= his[np.maximum(j, 0)]))[0]
    inside = R.membership(pairs)
    return [int(i) for i in cand if inside(R.value_of(words[i]))]


@functools.lru_cache(maxsize=None)
def oracle_set(name, n):
    """(pairs, the sorted records the oracle expects): a table of about 300 ranges around hashes of the first and the last 2048 keys"""
    offs, words, endos, types = records_of(name, n)
    near = np.nonzero((offs < 2048) | (offs >= n - 2048))[0]
    pairs = table_around([R.value_of(words[i]) for i in near], "%s %d" % (name, n))
    idx = member_indices(pairs, words)
    want = sorted(tuples_of(offs, words, endos, types, idx))
    if TYPES[name].get("eth"):  # every expected hit by eth_ref itself
        for off, w, e, _ in want:
            assert eth_by_reference(off, e) == list(w)
    assert 50 < len(want) < len(offs) // 10 and any(r[0] >= n - 2048 for r in want) and any(r[0] < 2048 for r in want)
    return pairs, want


def open_split(name, geometry=None, offs=0):
    from ecloop_amd import Device
    d = Device(0, ord_offs=offs, prefix=True, origin=True, **{"a33": True, **TYPES[name]})
    if geometry:
        d.set_geometry(*geometry)
    return d


def open_plain(name, geometry=None):
    from ecloop_amd import Device
    d = Device(0, prefix=True, **{"a33": True, **TYPES[name]})
    if geometry:
        d.set_geometry(*geometry)
    return d


# ---- flags through the C ABI

def test_flags_through_the_c_abi():
    from ecloop_amd import capi
    lib = capi.load()
    PO = capi.PREFIX | capi.ORIGIN
    A33, A65, E, ETH = capi.ADDR33, capi.ADDR65, capi.ENDO, capi.ETH
    good = [PO | A33, PO | A65, PO | A33 | A65, PO | ETH, PO | A33 | E, PO | A65 | E, PO | A33 | A65 | E, PO | ETH | E]
    for flags in good:  # the eight: each open runs the self-test of its own kernel selection, the walk from O = 0xdc2a04 G
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, flags, 0) == 0, flags
        lib.ecl_hip_close(h)
    bad = [PO, PO | E, PO | capi.PUB, PO | capi.PUB | E, PO | A33 | capi.PUB, PO | capi.TR, PO | capi.P2SH, PO | A33 | capi.P2SH, PO | A33 | ETH,
           PO | A33 | capi.INSERT, PO | A33 | capi.HERD, PO | A33 | 8, PO | A33 | 32, PO | A33 | 8192,
           capi.ORIGIN | A33, capi.ORIGIN | A33 | E, capi.ORIGIN | A65, capi.ORIGIN | ETH, capi.ORIGIN | capi.TR, capi.ORIGIN | capi.P2SH | A33, capi.ORIGIN,
           capi.PUB | capi.ORIGIN | E, capi.PUB | capi.ORIGIN | capi.INSERT]
    for flags in bad:
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, flags, 0) == capi.E_ARG, flags
    h = C.c_void_p()
    assert lib.ecl_hip_open(C.byref(h), 0, PO | A33, 0) == 0
    try:
        out, n = np.zeros(64, capi.FOUND_DTYPE), C.c_uint32()
        qx, qy = Q()
        start = np.concatenate([capi.limbs(A), capi.limbs(qx), capi.limbs(qy)])
        add = lambda s: lib.ecl_hip_add_range(h, s.ctypes.data, 2048, out.ctypes.data, 64, C.byref(n))
        assert add(start) == capi.E_NOBLOOM
        table = table_of([(0, 1 << 150)])
        assert lib.ecl_hip_set_bloom(h, table.ctypes.data, 5) == 0
        assert add(start) == 0
        first = keys_of(out[:n.value])
        ks = capi.limbs_array([1, 2, 3])
        assert lib.ecl_hip_mul_batch(h, ks.ctypes.data, 3, out.ctypes.data, 16, C.byref(n)) == capi.E_ARG
        text, lines = np.frombuffer(b"abc", np.uint8), np.array([3 << 32], np.uint64)
        assert lib.ecl_hip_mul_batch_raw(h, text.ctypes.data, 3, lines.ctypes.data, 1, out.ctypes.data, 16, C.byref(n)) == capi.E_ARG
        # an origin that is no point of the curve: refused, and the context is whole (the same call with the good origin gives the same records)
        for off_curve in ((qx, (qy + 1) % P), (P, qy), (qx, P), (0, 0)):
            s = np.concatenate([capi.limbs(A), capi.limbs(off_curve[0]), capi.limbs(off_curve[1])])
            assert add(s) == capi.E_ARG and n.value == 0
        assert add(start) == 0 and keys_of(out[:n.value]) == first
        # ... and so is a verify entry with such an origin
        h33, h65, ok = np.zeros((1, 5), np.uint32), np.zeros((1, 5), np.uint32), np.zeros(1, np.uint8)
        s = np.concatenate([capi.limbs(A), capi.limbs(qx), capi.limbs((qy + 1) % P)])
        assert lib.ecl_hip_verify(h, s.ctypes.data, 1, h33.ctypes.data, h65.ctypes.data, ok.ctypes.data) == capi.E_ARG
        assert lib.ecl_hip_verify(h, start.ctypes.data, 1, h33.ctypes.data, h65.ctypes.data, ok.ctypes.data) == 0 and ok[0] == 1
        assert [int(w) for w in h33[0]] == orc.hash160(*orc.point_of(KQ + A))
    finally:
        lib.ecl_hip_close(h)


# ---- exact-set parity

@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", list(TYPES))
def test_exact_set_parity_origin_walk_plain_walk_and_oracle(name, shape):
    """fails on the parent commit: ecl_hip_open refuses the flag combination there"""
    n = SHAPES[shape]
    pairs, want = oracle_set(name, n)
    table = table_of(pairs)
    d = open_split(name)
    try:
        d.set_prefixes(table)
        before = d.coverage()
        recs, total = d.add_range(A, n, cap=8192, origin=Q())
        after = d.coverage()
    finally:
        d.close()
    got = keys_of(recs)
    assert total == len(recs) and len(got) == len(set(got))
    assert tuple(b - a for a, b in zip(before, after)) == (n, n, n)
    p = open_plain(name)
    try:
        p.set_prefixes(table)
        precs, ptotal = p.add_range((KQ + A) % N, n, cap=8192)
    finally:
        p.close()
    plain = keys_of(precs)
    assert ptotal == len(precs)
    assert got == want and plain == want  # all three equal: key_offset, h160, endo, compressed


# ---- continuation, re-positioning, the base point that is -O

def test_continuation_and_another_origin_repositions():
    n1, n2 = 4096, 8192  # whole sweeps of the 8 x 256 geometry, so the resident walk can go on
    pairs, _ = oracle_set("c", SHAPES["5000"])
    offs, words, endos, types = records_of("c", SHAPES["2^17+3"])
    first = np.nonzero(offs < n1 + n2)[0]
    want = sorted(tuples_of(offs, words, endos, types, [first[i] for i in member_indices(pairs, words[first])]))
    assert len(want) > 50
    other_k = KQ + 0x1234567
    O2 = orc.point_of(other_k)
    d = open_split("c", (8, 256))
    try:
        d.set_prefixes(table_of(pairs))
        one, _ = d.add_range(A, n1 + n2, cap=4096, origin=Q())
        assert keys_of(one) == want
        d.reset_timing()
        a, _ = d.add_range(A, n1, cap=4096, origin=Q())
        b, _ = d.add_range(A + n1, n2, cap=4096, origin=Q())  # contiguous, same origin: the resident walk goes on
        assert d.setup_timing()[1] == 1
        b = b.copy()
        b["key_offset"] += n1
        assert keys_of(np.concatenate([a, b])) == want and len(a) and len(b)
        # the scalar that would continue, with another origin: re-positioned, and the records are that origin's
        c, _ = d.add_range(A + n1 + n2, n1, cap=4096, origin=O2)
        assert d.setup_timing()[1] == 2
        p = open_plain("c", (8, 256))
        try:
            p.set_prefixes(table_of([(0, R.TOP >> 6)]))
            d.set_prefixes(table_of([(0, R.TOP >> 6)]))
            c, _ = d.add_range(A + n1 + n2 + n1, n1, cap=4096, origin=O2)  # (continues O2's walk: contiguous, same origin)
            assert d.setup_timing()[1] == 2
            pc, _ = p.add_range((other_k + A + n1 + n2 + n1) % N, n1, cap=4096)
            assert keys_of(c) == keys_of(pc) and 20 < len(c) < 200
            # the first origin again, at the scalar that continues the call before: starts anew, with the first origin's records
            e, _ = d.add_range(A + n1 + n2 + 2 * n1, n1, cap=4096, origin=Q())
            assert d.setup_timing()[1] == 3
            pe, _ = p.add_range((KQ + A + n1 + n2 + 2 * n1) % N, n1, cap=4096)
            assert keys_of(e) == keys_of(pe) and keys_of(e) != keys_of(c) and len(e) > 20
        finally:
            p.close()
    finally:
        d.close()


def test_a_base_point_that_is_minus_the_origin_is_a_range_error():
    """an error return, as in tests/test_gpu_bsgs.py - nothing faults: k_origin_add raises its flag, the call reports ECL_E_RANGE and no records"""
    from ecloop_amd import EclError
    s, n = 0x7000, 4096
    geometry = (8, 256)  # the walk's base point E = (s + B - 2B) G = (s - 8) G
    ex, ey = orc.point_of(s - 8)
    d = open_split("c", geometry)
    try:
        d.set_prefixes(WHOLE)
        good, total = d.add_range(s, n, cap=n, origin=Q())
        assert total == n
        with pytest.raises(EclError) as err:
            d.add_range(s, n, cap=n, origin=(ex, P - ey))
        assert err.value.code == -6
        assert len(d.fetch_found(0, 16)) == 0  # no records
        again, total = d.add_range(s, n, cap=n, origin=Q())  # the next ordinary call is correct
        assert total == n and keys_of(again) == keys_of(good)
        h33, _, ok = orc.mul_hash160_many(scalars_le([KQ + s + j for j in range(n)]), True, False)
        assert sorted((int(r["key_offset"]), tuple(int(w) for w in r["h160"])) for r in again) == sorted((j, tuple(int(w) for w in h33[j])) for j in range(n))
    finally:
        d.close()


# ---- overflow, fetch, keys past nkeys

@pytest.mark.parametrize("name", ["cu-endo", "e"])
def test_dense_hits_overflow_fetch_and_no_record_past_nkeys(name):
    n = 3000  # not a multiple of the group: the last group's keys past nkeys must not be reported
    offs, words, endos, types = records_of(name, SHAPES["5000"])
    want = sorted(tuples_of(offs, words, endos, types, np.nonzero(offs < n)[0]))
    d = open_split(name, (8, 256))
    try:
        d.set_prefixes(WHOLE)
        recs, total = d.add_range(A, n, cap=len(want) + 16, origin=Q())
        assert total == len(recs) == len(want) and keys_of(recs) == want and max(int(r["key_offset"]) for r in recs) == n - 1
        assert d.coverage() == (n, n, n)
        first, total = d.add_range(A, n, cap=16, origin=Q())  # ECL_E_OVERFLOW: the true total, sixteen records, the rest still on the device
        assert total == len(want) and len(first) == 16
        rest = d.fetch_found(16, total - 16)
        assert len(rest) == total - 16 and keys_of(np.concatenate([first, rest])) == want
    finally:
        d.close()


# ---- k_verify_origin / k_verify_origin_eth

def verify_cases():
    """65 entries - a full wave and a tail: (k, origin or None, the key of the sum or None for the point at infinity)"""
    from ecloop_amd.engine import calc_priv
    rng = random.Random("verify origin")
    cases = []
    for i in range(40):  # random k, a per-entry origin
        k, ko = rng.randrange(1, N), rng.randrange(1, N)
        cases.append((k, orc.point_of(ko), (k + ko) % N))
    for e in range(1, 6):  # image origins: the entry (k', O') of image e of Q + k G, whose key is calc_priv(KQ + k, e)
        for _ in range(2):
            k = rng.randrange(1, 1 << 200)
            cases.append((calc_priv(k, 1, 0, e), image_point(Q(), e), calc_priv(KQ + k, 1, 0, e)))
    k = rng.randrange(1, N)
    cases.append((k, orc.point_of(k), 2 * k % N))  # k G = O: the doubling
    cases.append((k, orc.point_of(N - k), None))  # k G = -O: the point at infinity, ok = 0
    cases.append((5, orc.point_of(N - 5), None))
    for zero_digit in (1 << 14, (1 << 28) | 5, (rng.randrange(1, N) >> 42 << 42) | 0x3FFF, 1 << 252, (1 << 252) | (0x3FFF << 14)):  # zero window digits (14-bit windows)
        cases.append((zero_digit, Q(), (zero_digit + KQ) % N))
    cases.append((0, Q(), KQ))  # k = 0: every digit zero, the sum is O
    cases.append((N, Q(), KQ))  # k = n: the window sum itself is the point at infinity, then + O
    cases.append((7, None, 7))  # O at infinity: k G alone
    cases.append((0, None, None))  # k = 0 with O at infinity
    cases.append((N, None, None))
    while len(cases) < 65:
        k, ko = rng.randrange(1, N), rng.randrange(1, N)
        cases.append((k, orc.point_of(ko), (k + ko) % N))
    assert len(cases) == 65
    return cases


def test_verify_origin_kernels_against_the_oracle():
    cases = verify_cases()
    ks, orgs = [c[0] for c in cases], [c[1] for c in cases]
    d = open_split("c")
    try:
        h33, h65, ok = d.verify(ks, origin=orgs)
    finally:
        d.close()
    d = open_split("e")
    try:
        addr, oke = d.verify_eth(ks, origin=orgs)
        one33, _, ok1 = d.verify(ks[:3], origin=orgs[0])  # one point for all; any split-key context answers both calls
    finally:
        d.close()
    for i, (k, o, key) in enumerate(cases):
        assert int(ok[i]) == int(oke[i]) == (0 if key is None else 1), (i, k, o)
        if key is None:
            continue
        x, y = orc.point_of(key)
        assert [int(w) for w in h33[i]] == orc.hash160(x, y, True), i
        assert [int(w) for w in h65[i]] == orc.hash160(x, y, False), i
        assert [int(w) for w in addr[i]] == eth_ref.eth_words(x, y), i
    for i in range(3):
        assert ok1[i] and [int(w) for w in one33[i]] == orc.hash160(*orc.point_of((ks[i] + cases[0][2] - cases[0][0]) % N))


def test_verify_on_an_ordinary_context_is_untouched():
    from ecloop_amd import Device
    ks = [1, 2, 0xDC2A04, N - 1, 0]
    for d in (Device(0), open_plain("c")):
        try:
            h33, h65, ok = d.verify(ks)
            addr, oke = d.verify_eth(ks)
            with pytest.raises(ValueError):
                d.verify(ks, origin=Q())
        finally:
            d.close()
        assert [int(v) for v in ok] == [int(v) for v in oke] == [1, 1, 1, 1, 0]
        for i, k in enumerate(ks[:4]):
            x, y = orc.point_of(k)
            assert [int(w) for w in h33[i]] == orc.hash160(x, y, True) and [int(w) for w in h65[i]] == orc.hash160(x, y, False)
            assert [int(w) for w in addr[i]] == eth_ref.eth_words(x, y)


# ---- coverage

def test_drop_round_fails_an_origin_call_and_the_next_is_whole():
    from ecloop_amd import EclError
    n = 4096
    d = open_split("c", (8, 256))
    try:
        d.set_prefixes(WHOLE)
        first, total = d.add_range(A, n, cap=n, origin=Q())
        assert total == n
        cov = d.coverage()
        d.diag_drop_round()
        with pytest.raises(EclError) as e:
            d.add_range(A + n, n, cap=n, origin=Q())
        assert e.value.code == -8
        now = d.coverage()
        assert now[0] - cov[0] == n and now[1] == cov[1] and now[2] - cov[2] < n
        recs, total = d.add_range(A + n, n, cap=n, origin=Q())
        assert total == len(recs) == n
        h33, _, _ = orc.mul_hash160_many(scalars_le([KQ + A + n + j for j in range(n)]), True, False)
        assert sorted((int(r["key_offset"]), tuple(int(w) for w in r["h160"])) for r in recs) == sorted((j, tuple(int(w) for w in h33[j])) for j in range(n))
    finally:
        d.close()


# ---- the engine

def test_engine_prefix_search_with_an_origin():
    from ecloop_amd.engine import prefix_search, splitkey_combine
    lo, n = 0x10000, 1 << 16
    h33, _, _ = orc.mul_hash160_many(scalars_le([KQ + lo + j for j in range(n)]), True, False)
    known = R.value_of(h33[1234])
    pattern = R.p2pkh(known)[:4]  # "1" and three digits: 58^-3, inside the planner's bound of 2^-16
    want = sorted((lo + j, R.p2pkh(R.value_of(h))) for j, h in enumerate(h33) if R.p2pkh(R.value_of(h)).startswith(pattern))
    assert (lo + 1234, R.p2pkh(known)) in want
    recs, edge = prefix_search([pattern], lo, lo + n, origin=Q())
    assert sorted((r.pk, r.address) for r in recs) == want and edge == 0 and all(r.split == 0 for r in recs)
    for r in recs:  # the partial key is worthless alone; combined with k_Q it is the key of the printed address
        final = splitkey_combine(KQ, r.pk, r.split)
        assert R.p2pkh(R.value_of(orc.hash160(*orc.point_of(final)))) == r.address
        assert r.line().endswith("\t%s\tsplit:0" % r.address) and r.stdout_line().endswith(" %s split:0" % r.address)


# ---- the CLI

LO, HI = 0xD00000, 0xE00000  # -r d00000:dfffff: 2^20 keys


def pub_hex(pt):
    return "%02x%064x" % (2 | (pt[1] & 1), pt[0])


@pytest.fixture(scope="module")
def image_hashes():
    """the oracle's addr33 hashes of the six images of the 2^20 points Q + k G, k = LO ... HI - 1: [e] -> (n, 5) uint32; and the partial keys"""
    from ecloop_amd.engine import LAMBDA
    n = HI - LO
    out, parts = [], []

    def run(first, step):  # first, first + step, ... (mod n): n scalars as little-endian limbs
        vals, v = [], first
        for _ in range(n):
            vals.append(v)
            v += step
            if v >= N:
                v -= N
        return vals
    K0 = (KQ + LO) % N
    l2 = LAMBDA * LAMBDA % N
    for e in range(6):
        m = (1, LAMBDA, l2)[e // 2]
        sign = N - 1 if e & 1 else 1
        keys = run(K0 * m * sign % N, m * sign % N)
        h33, _, ok = orc.mul_hash160_many(scalars_le(keys), True, False)
        assert ok.all()
        out.append(h33)
        parts.append((LO * m * sign % N, m * sign % N))  # partial key of offset j: first + j * step
    return out, parts


def p2pkh_candidates(h, pattern):
    """indices whose P2PKH address can start with the pattern ("1" and three base58 digits): the leading digits of the 25-byte number from the
    leading 64 bits of the hash in floating point, one unit of slack either way; the caller encodes the candidates exactly"""
    top = ((h[:, 0].astype(np.uint64) << np.uint64(32)) | h[:, 1].astype(np.uint64)).astype(np.float64)
    L = (np.log(np.maximum(top, 1.0)) + 128 * np.log(2.0)) / np.log(58.0)  # log58 of hash * 2^32
    head = np.floor(np.power(58.0, L - np.floor(L) + len(pattern) - 2))
    want = 0
    for c in pattern[1:]:
        want = want * 58 + R.B58.index(c)
    return np.nonzero(np.abs(head - want) <= 1)[0]


def test_cli_add_split_key_lines_combine_and_rnd(cli, image_hashes, tmp_path):
    """fails on the parent commit: there `add` ignores -k and prints whole keys for the points k G"""
    from ecloop_amd.engine import prefix_ranges, splitkey_combine
    hashes, parts = image_hashes
    n = HI - LO
    j0 = 0xC2A04  # a known point of the walk: its image 3 gives the base58 pattern, image 4 of another one the bech32 pattern
    v0, v1 = R.value_of(hashes[3][j0]), R.value_of(hashes[4][j0 + 77])
    p58, bech = R.p2pkh(v0)[:4], R.p2wpkh(v1)[:9]
    patterns = [p58, bech]
    hits = []  # (hash value, partial key, address, e), by brute force over the oracle's hashes: every address encoded, no range arithmetic
    top = v1 >> 135
    for e in range(6):
        h = hashes[e]
        first, step = parts[e]
        for j in p2pkh_candidates(h, p58):
            v = R.value_of(h[j])
            if R.p2pkh(v).startswith(p58):
                hits.append((v, (first + int(j) * step) % N, R.p2pkh(v), e))
        for j in np.nonzero(h[:, 0] >> np.uint32(7) == top)[0]:
            v = R.value_of(h[j])
            if R.p2wpkh(v).startswith(bech) and not R.p2pkh(v).startswith(p58):
                hits.append((v, (first + int(j) * step) % N, R.p2wpkh(v), e))
    assert (v0, (parts[3][0] + j0 * parts[3][1]) % N, R.p2pkh(v0), 3) in hits and len(hits) >= 10
    want = sorted("addr33: %040x <- %064x %s split:%d" % h for h in hits)
    # edge: records inside the planned ranges whose text matches no pattern
    table, _ = prefix_ranges(patterns, True, False, False)
    pairs = [(R.value_of(r[:5]), R.value_of(r[5:])) for r in table]
    inside = sum(len(member_indices(pairs, h)) for h in hashes)
    edge = inside - len(hits)
    assert 0 <= edge < 4
    f = tmp_path / "patterns.txt"
    f.write_text("%s\n%s\n" % (p58, bech))
    outfile = tmp_path / "found.txt"
    args = ["-p", str(f), "-k", pub_hex(Q()), "-a", "c", "-endo", "-r", "%x:%x" % (LO, HI - 1)]
    r = run_cli(cli, ["add"] + args + ["-o", str(outfile)], timeout=300)
    assert r.found == want, (r.stdout, r.status)
    assert "edge: %d" % edge in r.status and "filter: prefix (2 patterns, " in r.stdout
    assert "PARTIAL keys for %s" % pub_hex(Q()) in r.stdout
    assert sorted(outfile.read_text().splitlines()) == sorted("addr33\t%040x\t%064x\t%s\tsplit:%d" % h for h in hits)  # a fifth tab-separated field
    # the requester's side: every partial key combined with k_Q is the key of the printed address (combine prints it, and its addresses)
    for v, part, address, e in hits:
        final = splitkey_combine(KQ, part, e)
        assert R.value_of(orc.hash160(*orc.point_of(final))) == v
    for v, part, address, e in hits[:3] + [h for h in hits if h[3] == 3][:1]:
        pr = subprocess.run([cli, "combine", "-part", "%064x" % part, "-split", str(e)], input=("%x\n" % KQ).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        lines = pr.stdout.decode().splitlines()
        assert pr.returncode == 0 and lines[0] == "key: %064x" % splitkey_combine(KQ, part, e), pr.stderr.decode()[-1000:]
        assert lines[1].startswith("addr33: %040x " % v) and address in lines[1].split()[2:]
    # rnd: one window with a fixed seed; it walks the 2^21 keys from d00000 (full-size jobs), so the lines of `add` are among its lines,
    # and every line's partial key, combined, gives its address
    r = run_cli(cli, ["rnd"] + args[:-2] + ["-seed", "splitkey", "-r", "%x:%x" % (LO, HI - 1), "-d", "0:20"], env={"ECLOOP_HIP_RND_WINDOWS": "1"}, timeout=300)
    assert set(want) <= set(r.found), (r.stdout, r.status)
    for line in r.found:
        _, h, _, k, a, sp = line.split()
        final = splitkey_combine(KQ, int(k, 16), int(sp.split(":")[1]))
        v = R.value_of(orc.hash160(*orc.point_of(final)))
        assert "%040x" % v == h and a in (R.p2pkh(v), R.p2wpkh(v)) and (a.startswith(p58) or a.startswith(bech))
