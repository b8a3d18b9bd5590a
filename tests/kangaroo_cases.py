"""The inputs of tests/test_gpu_kangaroo_wide.py, constructed: herd blocks at which the kernel's rarely used paths are in use - the upper
words of the distance, distinguished points decided by limb 1 of x, calls of more than one launch, a herd of two set-up chunks, starts at
the point at infinity, zero offsets, a distance that passes 2^128, a base above 2^128.  Pure Python over tests/kangaroo_ref.py and the
oracle's points; tests/test_kangaroo_cases.py asserts, without a GPU, that every input has the property it was made for.  Test
infrastructure only."""
import functools
import random

import kangaroo_ref as ref
import orc

P, N = orc.P, orc.N
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
KEY, BASE = 0x123456789, 0x100000000
WIDE_BASE = (1 << 200) + 0x1234567


def neg(pt):
    return pt[0], (P - pt[1]) % P


def words_of(d):
    return [(d >> (32 * w)) & M32 for w in range(4)]


# ---- A: wide distances -----------------------------------------------------------------------------------------------------------
# id -> (herd_log2, seed, jb, sb, dp, steps), all with WIDE_BASE and the target KEY G
WIDE = {"H2": (1, 3, 90, 100, 3, 300), "H128": (7, 9, 90, 100, 3, 100), "H4096": (12, 5, 90, 100, 3, 64), "H128-carry": (7, 9, 64, 64, 0, 16)}


def wide_block(name):
    hl, seed, jb, sb, _, _ = WIDE[name]
    return WIDE_BASE, orc.point_of(KEY), seed, hl, jb, sb


@functools.lru_cache(maxsize=None)
def wide_run(name):
    """-> (the sorted records of Herd.run, what they exercise): the records whose distance has word 2 / word 3 in use, the recorded jumps in
    which word 1 carried into word 2, and the table's distances of 2^64 and more"""
    hl, seed, jb, sb, dp, steps = WIDE[name]
    herd = ref.Herd(*wide_block(name))
    out, seen = [], {"word2": 0, "word3": 0, "carry": 0, "table_hi": sum(1 for s in herd.s if s >> 64)}
    for _ in range(steps):
        before = list(herd.d)
        recs = herd.step(dp)
        out += recs
        marked = [i for i in range(herd.H) if not herd.x[i] & ((1 << dp) - 1)]
        assert len(marked) == len(recs)
        for i in marked:
            w = words_of(herd.d[i])
            seen["word2"] += w[2] != 0
            seen["word3"] += w[3] != 0
            seen["carry"] += (herd.d[i] & M64) < (before[i] & M64)  # the low half wrapped: the sum of words 0, 1 carried
    return tuple(sorted(out)), seen


# ---- B: distinguished points across the limb boundary ----------------------------------------------------------------------------
DP_HERD = (3, 7, 90, 100)  # seed, herd_log2, jb, sb
DP_STEPS = 8
# name -> (zero low bits, the bit above them set, [(dp the context is opened with, a record is expected)])
DP_TARGETS = {"Z32": (32, False, [(29, True), (30, True), (31, True), (32, True)]), "Z31": (31, True, [(31, True), (32, False)]),
              "Z29": (29, True, [(29, True), (30, False)]), "Z28": (28, True, [(28, True), (29, False)])}


def lift(x):
    """a point with this x, or None (p = 3 mod 4: the root of a square is its (p + 1) / 4-th power)"""
    c = (x * x * x + 7) % P
    y = pow(c, (P + 1) // 4, P)
    return (x, y) if y * y % P == c else None


@functools.lru_cache(maxsize=None)
def dp_target(name):
    """-> (block, j, X*): a target Q for which wild kangaroo 1 starts on S = X* - T_j with j the index S.x picks, so that its first jump
    lands on X*, a point whose x has the low bits of the name"""
    z, top, _ = DP_TARGETS[name]
    seed, hl, jb, sb = DP_HERD
    s, r = ref.distances_and_offsets(seed, hl, jb, sb)
    T = [orc.point_of(v) for v in s]
    rnd = random.Random("kangaroo dp " + name)
    while True:
        x = (rnd.getrandbits(256) >> (z + 1) << (z + 1) | (1 << z if top else 0)) % P
        star = lift(x)
        if star is None or x & ((1 << z) - 1) or bool(x >> z & 1) != top:
            continue
        for j in range(32):
            S = ref.add_points(star, neg(T[j]))
            if S is not None and (S[0] >> 32) & 31 == j and S[0] != T[j][0]:
                q = ref.add_points(S, neg(orc.point_of(r[1]))) if r[1] else S
                if q is not None:
                    return (WIDE_BASE, q, seed, hl, jb, sb), j, star


@functools.lru_cache(maxsize=None)
def dp_run(name, dp):
    return tuple(sorted(ref.Herd(*dp_target(name)[0]).run(DP_STEPS, dp)))


# ---- C: calls of more than one launch --------------------------------------------------------------------------------------------
LAUNCH_STEPS_MAX = 4096  # HERD_LAUNCH_STEPS_MAX of csrc/abi_herd.h
# id -> (herd_log2, seed, jb, sb, dp, steps)
LONG = {"H2": (1, 3, 20, 30, 3, 2 * LAUNCH_STEPS_MAX + 7), "H32": (5, 9, 20, 30, 3, LAUNCH_STEPS_MAX + 1)}
LONG_SPLIT = (LAUNCH_STEPS_MAX + 1, LAUNCH_STEPS_MAX + 6)  # the steps of H2 again, as two contiguous calls of more than one launch each


def long_block(name):
    hl, seed, jb, sb, _, _ = LONG[name]
    return BASE, orc.point_of(KEY), seed, hl, jb, sb


@functools.lru_cache(maxsize=None)
def long_run(name):
    return tuple(sorted(ref.Herd(*long_block(name)).run(LONG[name][5], LONG[name][4])))


# ---- D: a herd of two set-up chunks ----------------------------------------------------------------------------------------------
INIT_CHUNK = 1 << 18  # HERD_INIT_CHUNK of csrc/abi_herd.h
BIG = (19, 11, 20, 60)  # herd_log2, seed, jb, sb; dp = 0, one step


def big_block():
    hl, seed, jb, sb = BIG
    return BASE, orc.point_of(KEY), seed, hl, jb, sb


@functools.lru_cache(maxsize=None)
def big_herd():
    """-> (the 32 distances, the 2^19 offsets)"""
    hl, seed, jb, sb = BIG
    return ref.distances_and_offsets(seed, hl, jb, sb)


def big_sample():
    H = 1 << BIG[0]
    rnd = random.Random("kangaroo two chunks")
    edges = [0, 1, 2, 3, INIT_CHUNK - 2, INIT_CHUNK - 1, INIT_CHUNK, INIT_CHUNK + 1, H - 2, H - 1]
    rest = set()
    while len(rest) < 54:
        i = rnd.randrange(H)
        if i not in edges:
            rest.add(i)
    return edges + sorted(rest)


@functools.lru_cache(maxsize=None)
def big_expected():
    """-> {i: the record of kangaroo i's first jump}, i over the sample: its start by the oracle, one jump by the yardstick's rule"""
    base, q, _, _, _, _ = big_block()
    s, r = big_herd()
    T = [orc.point_of(v) for v in s]
    out = {}
    for i in big_sample():
        _, pt, d = ref.jump_of(s, T, ref.start_of(base, q, r[i], i), r[i])
        out[i] = ref.record(i, d, pt[0])
    return out


# ---- E: the refusals and the odd starts ------------------------------------------------------------------------------------------
ODD = (9, 7, 20, 30)  # seed, herd_log2, jb, sb of the two herds with a start at infinity, and of the good block that follows
ODD_GOOD_STEPS = 50


def odd_good_block():
    seed, hl, jb, sb = ODD
    return BASE, orc.point_of(KEY), seed, hl, jb, sb


@functools.lru_cache(maxsize=None)
def odd_good_run():
    return tuple(sorted(ref.Herd(*odd_good_block()).run(ODD_GOOD_STEPS, 3)))


def wild_infinity_block():
    """Q = (n - r_1) G: wild kangaroo 1 starts on Q + r_1 G, the point at infinity"""
    seed, hl, jb, sb = ODD
    _, r = ref.distances_and_offsets(seed, hl, jb, sb)
    return BASE, orc.point_of(N - r[1]), seed, hl, jb, sb


def tame_infinity_block():
    """base = n - r_0: tame kangaroo 0 starts on (base + r_0) G, the point at infinity"""
    seed, hl, jb, sb = ODD
    _, r = ref.distances_and_offsets(seed, hl, jb, sb)
    return N - r[0], orc.point_of(KEY), seed, hl, jb, sb


ZERO = (5, 7, 10, 1, 0, 64)  # seed, herd_log2, jb, sb, dp, steps: every offset is 0 or 1


def zero_block():
    seed, hl, jb, sb, _, _ = ZERO
    return BASE, orc.point_of(KEY), seed, hl, jb, sb


@functools.lru_cache(maxsize=None)
def zero_run():
    return tuple(sorted(ref.Herd(*zero_block()).run(ZERO[5], ZERO[4])))


OVER = (1, 1, 120, 124)  # seed, herd_log2, jb, sb; dp = 0


def over_block():
    seed, hl, jb, sb = OVER
    return WIDE_BASE, orc.point_of(KEY), seed, hl, jb, sb


@functools.lru_cache(maxsize=None)
def over_run():
    """-> (k, the sorted records of the k - 1 steps before it): step k is the one in which Herd.step raises OverflowError"""
    herd, out, k = ref.Herd(*over_block()), [], 0
    while True:
        k += 1
        try:
            out += herd.step(0)
        except OverflowError:
            return k, tuple(sorted(out))
        assert k < 10000


# ---- F: end to end at a wide base ------------------------------------------------------------------------------------------------
FAR_A = (1 << 200) + 0x7000000000
FAR_B = FAR_A + (1 << 32) - 1
FAR_KEY = FAR_A + 0x3C0FFEE1
FAR_OPTIONS = {"herd_log2": 8, "dp_bits": 5, "seed": 1, "round_steps": 64}


@functools.lru_cache(maxsize=None)
def far_search():
    return ref.search(orc.point_of(FAR_KEY), FAR_A, FAR_B, **FAR_OPTIONS)
