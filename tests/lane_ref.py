"""The lane set-up of a non-contiguous `add` call at the lane counts the product runs (2^18 ... 2^21) and calls past 2^32 keys: which
lanes to look at, which keys of them to plant in the filter, and what the call must then report.  The reference of
tests/test_gpu_lane_setup.py; CPU only, checked by tests/test_lane_ref.py.

A filter that holds nothing but the planted keys turns a call of 2^21 ... 2^33 keys into an exact check: the records must be the planted
set, each once.  Only the planted keys need a reference - orc.mul_hash160_many over their scalars (cmd_mul's path of the oracle: no walk,
no lane, nothing of the device), or tests/pub_ref.py's leading words of x for an origin context.  The filter is filled on the CPU
(orc_blf_add_many, as tests/test_gpu_blf.py fills its expectation).

Why set equality is sound: at most CAP = 4096 entries set at most 20 * 4096 of the filter's 2^26 bits, a density below 0.002 (asserted
on the filter that is used, not on the kernel).  A key that was not planted passes 20 probes with probability below 0.002^20 ~ 10^-54;
over the 2^33 keys of the largest call that is below 10^-44."""
import ctypes as C

import numpy as np

import orc
import pub_ref
import walk_ref
from ecloop_amd.capi import limbs_array

N = orc.N
CAP = 4096                # planted entries per call, at most
FILTER_WORDS = 1 << 20    # 2^26 bits
DENSITY = 0.002
SEED = 0x1A9E5            # of the seeded lanes, offsets and starts


def exceptional_start(B, offs, m):
    """the start k0 for which E = C0 - D is the table point of lane m: C0 = (k0 + B s) G, D = 2B s G, s = 2^offs, and
    k0 + B s - 2B s = (m + 1) 2B s  <=>  k0 = (2m + 3) B s.  Lane m's centre is then the doubling 2 (m + 1) D."""
    return (2 * m + 3) * B << offs


def per_thread_of(T):
    """lanes per thread of k_init_centres_table: four while the walk is small, eight from 2^19 lanes on"""
    return 8 if T >= 1 << 19 else 4


def thread_lanes(T, per_thread, m):
    """the lanes of lane m's thread in k_init_centres_table<per_thread>: r nt + t, nt = T / per_thread"""
    nt = T // per_thread
    return [r * nt + m % nt for r in range(per_thread)]


def lanes_of_interest(T, per_thread, m=None):
    """the lanes a call of T lanes is looked at, sorted: the ends, the seams between the threads of k_init_centres_table<per_thread>
    (g = r nt + t) and of k_init_centres_batched (g0 = 16 t), every power of two with its neighbours (the ladder's bits), 64 seeded
    lanes, and - m given - the exceptional lane, its neighbours and the whole of its thread"""
    assert T % 256 == 0 and T % per_thread == 0
    nt = T // per_thread
    lanes = {0, 1, T - 1, nt - 1, nt, nt + 1}
    lanes |= {r * nt + t for r in range(per_thread) for t in (0, nt - 1)}
    lanes |= {g + d for j in range(T.bit_length()) if (1 << j) < T for g in (1 << j,) for d in (-1, 0, 1)}
    rnd = [int(g) for g in np.random.default_rng(SEED).integers(0, T, 64)]
    lanes |= set(rnd)
    for g in [15, T // 2, T - 16] + rnd[:8]:  # the batched kernel's seams: the last lane of one thread, the first of the next
        lanes |= {16 * (g // 16) + 15, 16 * (g // 16) + 16}
    if m is not None:
        lanes |= {m - 1, m, m + 1} | set(thread_lanes(T, per_thread, m))
    return sorted(g for g in lanes if 0 <= g < T)


def lanes_and_rounds(nkeys, B, Tmax):
    """(lanes, groups per lane) of a call of nkeys keys at half group B on a context of at most Tmax lanes: the fewest rounds, then the
    fewest lanes (a multiple of 256) that cover the groups"""
    ngroups = -(-nkeys // (2 * B))
    nb = -(-ngroups // Tmax)
    return min(Tmax, (-(-ngroups // nb) + 255) & ~255), nb


def planted(start, offs, B, T, nb, lanes, nkeys, extra_offsets=()):
    """the key offsets to plant, sorted and unique (uint64): the first, the centre and the last key of the group of every lane of `lanes`
    in every round (walk_ref.group_offsets), clipped to nkeys, and extra_offsets.  No planted key may be the scalar 0."""
    offs_ = set(int(o) for o in extra_offsets)
    for rnd in range(nb):
        for g in lanes:
            grp = walk_ref.group_offsets(B, T, g, rnd)
            offs_ |= {grp[0], grp[B], grp[-1]}
    out = sorted(o for o in offs_ if 0 <= o < nkeys)
    assert all((start + (o << offs)) % N for o in out)
    return np.array(out, np.uint64)


def scalars_of(start, offs, offsets, t=0):
    return [(start + (int(o) << offs) + t) % N for o in offsets]


def _records(offsets, words, rtype):
    rec = np.zeros(len(offsets), walk_ref.REC)
    rec["key_offset"], rec["type"], rec["h160"] = offsets, rtype, words
    return walk_ref.canon(rec)


def expected_hashing(start, offs, offsets):
    """what an addr33 context reports for the planted offsets: the hash of the compressed key of (start + off 2^offs) mod n"""
    h33, _, ok = orc.mul_hash160_many(limbs_array(scalars_of(start, offs, offsets)))
    assert ok.all()
    return _records(offsets, h33, walk_ref.TYPE["c"])


def expected_origin(start, offs, t, offsets):
    """what a public-key context walking from the origin t G reports: the five leading words of x of (start + off 2^offs + t) G"""
    x, _, ok = orc.mul_points_many(limbs_array(scalars_of(start, offs, offsets, t)))
    assert ok.all()
    words = [pub_ref.words5(sum(int(v) << (64 * i) for i, v in enumerate(row))) for row in x]
    return _records(offsets, np.array(words, np.uint32).reshape(-1, 5), 5)


def planted_filter(hashes):
    """a filter of FILTER_WORDS words that holds these hashes and nothing else, filled by the oracle's blf_add; the two conditions that make
    set equality sound are asserted here"""
    h = np.ascontiguousarray(hashes, dtype=np.uint32).reshape(-1, 5)
    assert 0 < len(h) <= CAP
    words = np.zeros(FILTER_WORDS, np.uint64)
    L = orc.lib()
    L.orc_blf_add_many.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    L.orc_blf_add_many(words.ctypes.data, FILTER_WORDS, h.ctypes.data, len(h))
    assert density(words) < DENSITY
    return words


def density(words):
    return int(np.unpackbits(words.view(np.uint8)).sum()) / (64 * len(words))


def lanes_that_differ(got, want, B, T):
    """the lanes whose records are missing, extra or wrong in `got` (both walk_ref.canon arrays), sorted"""
    a, b = set(map(bytes, got)), set(map(bytes, want))
    bad = np.array([np.frombuffer(r, walk_ref.REC)[0]["key_offset"] for r in a ^ b], np.uint64)
    return sorted(set(int(o) // (2 * B) % T for o in bad))


# ---------------------------------------------------------------------------------------------------------------- the cases
def _m(T, r, t):
    return r * (T // per_thread_of(T)) + t


def _random_start(i):
    """a seeded 200-bit start"""
    rng = np.random.default_rng(SEED + 1 + i)
    return (1 << 199) | int.from_bytes(rng.bytes(24), "little")


class Call:
    """one add_range call of a case: its start, the exceptional lane (or None), the origin's scalar (or None) and extra offsets"""

    def __init__(self, label, start, m=None, t=None, extra=()):
        self.label, self.start, self.m, self.t, self.extra = label, start, m, t, tuple(extra)


class Case:
    """geometry None: the automatic one - B, T and nb are what plan_geometry says on the device; `auto` is what the defaults give on an
    MI355X with its memory free (half group, most lanes), for the CPU checks"""

    def __init__(self, nkeys, calls, geometry=None, offs=0, auto=None, cap=CAP + 16, device=None, extras=None):
        self.nkeys, self.make_calls, self.geometry, self.offs, self.auto = nkeys, calls, geometry, offs, auto
        self.cap, self.device, self.extras = cap, device or {}, extras

    def plan(self, Tmax=None):
        """(B, T, nb) on the CPU"""
        B, tmax = self.geometry or self.auto
        T, nb = lanes_and_rounds(self.nkeys, B, Tmax or tmax)
        return B, T, nb

    def calls(self, B, T, nb):
        return self.make_calls(self, B, T, nb)

    def offsets(self, call, B, T, nb):
        lanes = lanes_of_interest(T, per_thread_of(T), call.m)
        return planted(call.start, self.offs, B, T, nb, lanes, self.nkeys, call.extra)

    def expected(self, call, B, T, nb):
        off = self.offsets(call, B, T, nb)
        if call.t is not None:
            return expected_origin(call.start, self.offs, call.t, off)
        return expected_hashing(call.start, self.offs, off)


def _exceptional(slots):
    """calls at exceptional_start for the lanes r nt + t"""
    def make(case, B, T, nb):
        nt = T // per_thread_of(T)
        named = {"0": 0, "mid": nt // 2 + 1, "last": nt - 1}
        return [Call("r%d-t%s" % (r, t), exceptional_start(B, case.offs, r * nt + named[t]), m=r * nt + named[t]) for r, t in slots]
    return make


def _case_c(case, B, T, nb):
    return [Call("E-is-infinity", B), Call("start-9", B + 1), Call("random-200-bit", _random_start(0))]


def _case_d(case, B, T, nb):
    m = _m(T, 5, 12345)
    return [Call("r5", exceptional_start(B, 0, m), m=m), Call("random-200-bit", _random_start(1))]


def _case_f(case, B, T, nb):
    m = 7 * (T // 8) + 5
    return [Call("r7", (2 * m + 3) * B, m=m)]


G_K0 = 0x7_0000_0000


def _case_g(case, B, T, nb):
    """E's scalar is k0 + B - 2B; the origin t G makes E + O = (m + 1) D, and t + 1 moves it off every table point's x"""
    m = _m(T, 4, T // 16 + 1)
    t = ((m + 1) * 2 * B - (G_K0 - B)) % N
    return [Call("origin-r4", G_K0, m=m, t=t), Call("origin-plus-one", G_K0, t=(t + 1) % N)]


H_START = 0x1000000000


def past_2_32(B, T, nb, nkeys):
    """the extra offsets of the call of more than 2^32 keys: around 2^32, the last key, the first and last key of every round of lanes 0
    and T - 1, 64 seeded offsets above 2^32, and the first, centre and last key of 16 seeded groups above 2^32"""
    rng = np.random.default_rng(SEED + 7)
    out = {(1 << 32) - 1, 1 << 32, (1 << 32) + 1, nkeys - 1}
    for rnd in range(nb):
        for g in (0, T - 1):
            grp = walk_ref.group_offsets(B, T, g, rnd)
            out |= {grp[0], grp[-1]}
    out |= {int(o) for o in rng.integers(1 << 32, nkeys, 64)}
    for G in rng.integers((1 << 32) // (2 * B), -(-nkeys // (2 * B)), 16):
        out |= {int(G) * 2 * B + d for d in (0, B, 2 * B - 1)}
    return sorted(o for o in out if o < nkeys)


def _case_h(case, B, T, nb):
    return [Call("past-2^32", H_START, extra=past_2_32(B, T, nb, case.nkeys))]


H_KEYS = (1 << 32) + (1 << 22) + 5
CASES = {
    "a": Case(1 << 23, _exceptional([(r, t) for r in (0, 3, 4, 7) for t in ("0", "mid", "last")]), geometry=(8, 1 << 19)),
    "b": Case(1 << 22, _exceptional([(r, t) for r in (0, 3) for t in ("0", "last")]), geometry=(8, 1 << 18)),
    "c": Case(1 << 23, _case_c, geometry=(8, 1 << 19)),
    "d": Case(1 << 21, _case_d, geometry=(2, 1 << 19)),
    "e": Case(1 << 24, _exceptional([(6, "mid")]), geometry=(16, 1 << 19), offs=13, device=dict(ord_offs=13)),
    "f": Case(1 << 30, _case_f, auto=(256, 1 << 21)),
    "g": Case(1 << 23, _case_g, geometry=(8, 1 << 19), device=dict(a33=False, pub=True, origin=True)),
    "h": Case(H_KEYS, _case_h, auto=(1024, 1 << 21)),
    "i": Case(H_KEYS, _case_h, auto=(1024, 1 << 21), cap=16),
}
