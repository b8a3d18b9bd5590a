"""What every `mul` context must report for an array of scalars, computed once and shared: the reference of tests/test_gpu_mul_types.py.

For the scalars K[0 ... n - 1] a MulRef holds the 20 bytes a record of each type carries: addr33 / addr65 from orc.mul_hash160_many
(cmd_mul's 2048-scalar jobs restated), the points from orc.mul_points_many (the same workers), P2SH by tests/p2sh_ref.py over the addr33
hashes, Ethereum by eth_ref.keccak_many over x || y, the public-key type's five leading words of x, Taproot by tests/tr_ref.py's tweak and
affine formulas with the tweaks' points from one more orc.mul_points_many call and the inversions shared (Montgomery's trick).  Each table
is built when a context first asks for it.  records() gives a context's expectation for a call as a sorted walk_ref.REC array.

The scalars of the GPU test are here too (scalars()): seeded random 256-bit scalars with special ones planted at chosen (piece, round,
thread) positions of two call shapes.  geometry() and pieces() restate how ecl_hip_mul_batch cuts a call (csrc/abi_mul.h: mul_geometry,
mul_pieces), place() inverts them; tests/test_mul_ref.py asserts on the CPU that every planted scalar sits where it claims to, and checks
the tables against paths that share nothing with them."""
import functools

import numpy as np

import eth_ref
import orc
import p2sh_ref
import tr_ref
import walk_ref
from walk_ref import FILTER3, ONES, REC, canon, difference  # noqa: F401  (the GPU test takes them from here)

P, N = orc.P, orc.N
M256 = (1 << 256) - 1
TYPE = dict(walk_ref.TYPE, x=5)  # a record's `compressed` field
TABLE = dict(walk_ref.TABLE, x="pub")
# name -> (type letters, keyword arguments of capi.Device); `mul` ignores the endomorphism
CONTEXTS = {letters: (letters, dict(a33="c" in letters, a65="u" in letters, p2sh="s" in letters)) for letters in ("c", "u", "cu", "s", "cs", "us", "cus")}
CONTEXTS["e"] = ("e", dict(a33=False, eth=True))
CONTEXTS["t"] = ("t", dict(a33=False, tr=True))
CONTEXTS["x"] = ("x", dict(a33=False, pub=True))

# ---------------------------------------------------------------------------------------------- how a call is cut (csrc/abi_mul.h)
MUL_NT, MUL_R, MUL_CHUNK = 65536 * 3, 32, 1 << 22  # threads of a piece (ECL_MUL_WAVES = 3), scalars per thread at most, staging at most


def geometry(m):
    """mul_geometry: (scalars per thread R, threads nt) of one kernel launch over m scalars; scalar i is round i // nt of thread i % nt"""
    R = min(max(-(-m // MUL_NT), 1), MUL_R)
    return R, -(-(-(-m // R)) // 256) * 256


def pieces(n):
    """mul_pieces' cutting of a call of n scalars (below 2^26) on a context that has seen no longer call: [(at, m, R, nt, stream)]"""
    assert 0 < n < 1 << 26
    kbuf = 1 << 16
    while kbuf < MUL_CHUNK and kbuf < n:
        kbuf <<= 1
    top = min(kbuf, MUL_NT * 10)
    lim = min(top, MUL_NT)
    out, at = [], 0
    while at < n:
        m = min(n - at, lim)
        if n - at - m < lim // 2 and n - at <= kbuf and n - at <= MUL_NT * MUL_R:
            m = n - at  # no crumb at the end
        out.append((at, m) + geometry(m) + (len(out) % 2,))
        at += m
        lim = lim * 2 & ~1023 if lim * 2 <= top else top
    return out


def place(n, i):
    """scalar i of a call of n -> (piece, round, thread)"""
    for c, (at, m, R, nt, _) in enumerate(pieces(n)):
        if at <= i < at + m:
            return c, (i - at) // nt, (i - at) % nt
    raise IndexError(i)


def index_of(n, piece, rnd, thread):
    at, m, R, nt, _ = pieces(n)[piece]
    i = at + rnd * nt + thread
    assert rnd < R and thread < nt and i < at + m, (piece, rnd, thread)
    return i


# ---------------------------------------------------------------------------------------------- the scalars
def digit_edge_specials(W):
    """the digit patterns a W-bit window table can get wrong: every digit at its maximum, a single digit per window (1 and the maximum,
    the last window's narrower maximum included), 2^256 - 1, n - 1; and what the signed recoding turns on: a digit of exactly 2^(W-1)
    (the largest that stays positive), 2^(W-1) + 1 (the first that becomes negative with a carry), those in every window at once, a
    carry that runs through windows of all ones into the last row"""
    special = [M256, N - 1, N + 1, 1, 2]
    nwin = (256 + W - 1) // W
    for w in range(nwin):
        width = min(W, 256 - W * w)
        special += [1 << (W * w), ((1 << width) - 1) << (W * w), (((1 << width) - 1) << (W * w)) | 1]
        if width == W:
            half = 1 << (W - 1)
            special += [half << (W * w), (half + 1) << (W * w), ((half + 1) << (W * w)) | (M256 >> (W * (w + 1)) << (W * (w + 1)))]
    special += [sum((1 << (W - 1)) << (W * w) for w in range(nwin)) & M256, sum(((1 << (W - 1)) + 1) << (W * w) for w in range(nwin)) & M256,
                sum(((1 << (W - 1)) - 1) << (W * w) for w in range(nwin)) & M256]
    return special


def random_scalars(rng, n):
    return rng.integers(0, 1 << 63, (n, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.int64).astype(np.uint64)


def limbs(v):
    return [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]


def digit_edge_scalars(rng, n, W):
    """random 256-bit scalars with digit_edge_specials(W) in front"""
    K = random_scalars(rng, n)
    for i, v in enumerate(digit_edge_specials(W)):
        K[i] = limbs(v)
    return K


# Shape A: one piece of two scalars per thread whose second round ends inside a wave.  Shape B: a piece of one scalar per thread on the
# context's stream, then one of three per thread on the second stream with its own parking space; B's first NA scalars are A's.
NA = (1 << 18) + 77
NB = 196608 + 393216 + 5
WAVES = {("A", 0, 0): 100, ("A", 0, 1): 200, ("B", 1, 0): 1100, ("B", 1, 1): 1200, ("B", 1, 2): 1300}  # region -> first wave of its plantings
SHAPE_N = {"A": NA, "B": NB}


@functools.lru_cache(maxsize=None)
def scalars():
    """-> (K, planted): the (NB, 4) uint64 scalars of shape B (shape A: the first NA), and for every planted one
    (shape, piece, round, thread, kind, value, index)"""
    rng = np.random.default_rng(20261019)
    K = random_scalars(rng, NB)
    planted, taken = [], {}

    def put(shape, piece, rnd, thread, kind, value):
        i = index_of(SHAPE_N[shape], piece, rnd, thread)
        assert i not in taken, (shape, piece, rnd, thread, kind, taken.get(i))
        assert shape == "A" or i >= NA  # what B plants lies outside A
        taken[i] = kind
        K[i] = limbs(value)
        planted.append((shape, piece, rnd, thread, kind, value, i))

    inf = lambda j: (0, N)[j & 1]  # the two scalars without a point, in turn
    for (shape, piece, rnd), wave in WAVES.items():
        t = wave * 64
        put(shape, piece, rnd, t, "inf, lane 0", 0)
        put(shape, piece, rnd, t + 63, "inf, lane 63", N)
        for lane in range(64):
            put(shape, piece, rnd, t + 64 + lane, "inf, whole wave", inf(lane))
        put(shape, piece, rnd, t + 128 + 5, "inf, this round only", 0)
        put(shape, piece, rnd, t + 128 + 9, "inf, this round only", N)
        at = t + 192
        for W in (22, 26):
            for v in digit_edge_specials(W):
                put(shape, piece, rnd, at, "digit edge W=%d" % W, v)
                at += 1
        assert at <= t + 6 * 64
        for lane in range(64):  # short scalars take stand-in points and the complete sum; the long one keeps the wave's window loop running
            v = (1 << 250) | int(rng.integers(0, 1 << 60)) if lane == 17 else int(rng.integers(1, 1 << 40))
            put(shape, piece, rnd, t + 6 * 64 + lane, "short wave, long in lane 17", v)
        for lane in range(64):
            put(shape, piece, rnd, t + 7 * 64 + lane, "bit length %d" % (lane + 1), (1 << lane) | int(rng.integers(0, 1 << lane)) if lane else 1)
        for lane, v in enumerate([N - 1, N + 1, N + 12345, 2 * N & M256, M256, 1, 2]):
            put(shape, piece, rnd, t + 8 * 64 + lane, "around n", v)
    # every round of one thread
    for rnd in range(2):
        put("A", 0, rnd, 300 * 64 + 7, "inf, all rounds", inf(rnd))
    for rnd in range(3):
        put("B", 1, rnd, 1400 * 64 + 7, "inf, all rounds", inf(rnd))
    # threads whose later round is empty (A: round 1 ends at thread 130 892; B's second piece: round 2 at 130 564)
    put("A", 0, 0, 131000, "inf, later round empty", 0)
    put("B", 1, 0, 131000, "inf, later round empty", N)
    put("B", 1, 1, 131001, "inf, later round empty", 0)
    put("B", 1, 0, 131002, "inf, later round empty", 0)
    put("B", 1, 1, 131002, "inf, later round empty", N)
    # the last live lane of the partly filled wave of the last round
    put("A", 0, 1, NA - 1 - geometry(NA)[1], "inf, last live lane", N)
    at, m, R, nt, _ = pieces(NB)[1]
    put("B", 1, 2, m - 1 - 2 * nt, "inf, last live lane", 0)
    K.setflags(write=False)
    return K, tuple(planted)


# ---------------------------------------------------------------------------------------------- the tables
def ints_of(a):
    """(n, 4) uint64 little-endian limbs -> Python integers"""
    raw = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(a))]


def be_bytes(a):
    """(n, 4) uint64 little-endian limbs -> (n, 32) uint8, the numbers' big-endian bytes"""
    return np.ascontiguousarray(a[:, ::-1]).astype(">u8").view(np.uint8).reshape(len(a), 32)


def batch_inverse(vals):
    """the inverses mod p of non-zero integers by Montgomery's trick: one pow() for all of them"""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % P
    inv = pow(acc, -1, P)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % P
        inv = inv * vals[i] % P
    return out


class MulRef:
    def __init__(self, K):
        self.K = np.ascontiguousarray(K, dtype=np.uint64).reshape(-1, 4)
        self.n = len(self.K)

    @functools.cached_property
    def btc(self):
        return orc.mul_hash160_many(self.K, True, True)

    @functools.cached_property
    def h33(self):
        return self.btc[0]

    @functools.cached_property
    def h65(self):
        return self.btc[1]

    @functools.cached_property
    def ok(self):
        """1 where the scalar has a point (it is not 0 mod n)"""
        return self.btc[2].astype(bool)

    @functools.cached_property
    def points(self):
        """(x, y): (n, 4) uint64 limbs each, zero where ok is 0"""
        x, y, ok = orc.mul_points_many(self.K)
        assert np.array_equal(ok.astype(bool), self.ok)
        return x, y

    @functools.cached_property
    def p2sh(self):
        t = np.zeros((self.n, 5), np.uint32)
        for i in np.nonzero(self.ok)[0]:
            t[i] = p2sh_ref.p2sh_of_h33(self.h33[i])
        return t

    @functools.cached_property
    def eth(self):
        x, y = self.points
        digest = eth_ref.keccak_many(np.concatenate([be_bytes(x), be_bytes(y)], axis=1))
        words = np.ascontiguousarray(digest[:, 12:]).view(">u4").astype(np.uint32).reshape(self.n, 5)
        words[~self.ok] = 0
        return words

    @functools.cached_property
    def pub(self):
        """the five leading big-endian words of x (pub_ref.words5)"""
        return np.ascontiguousarray(be_bytes(self.points[0])[:, :20]).view(">u4").astype(np.uint32).reshape(self.n, 5)

    @functools.cached_property
    def tr(self):
        """the five leading words of the x of lift(P) + t G, t = tr_ref.tweak(P.x)"""
        live = np.nonzero(self.ok)[0]
        xs, ys = ints_of(self.points[0][live]), ints_of(self.points[1][live])
        ts = [tr_ref.tweak(x) for x in xs]
        assert all(0 < t < N for t in ts)  # (a tweak >= n: one key in 2^128 - BIP341 gives none, and neither does the device)
        tx, ty, tok = orc.mul_points_many(np.array([limbs(t) for t in ts], np.uint64).reshape(-1, 4))
        assert tok.all()
        txs, tys = ints_of(tx), ints_of(ty)
        ys = [y if y % 2 == 0 else P - y for y in ys]  # tr_ref.lift
        dx = [(b - a) % P for a, b in zip(xs, txs)]
        assert all(dx)  # lift(P) = +-t G: the sum would be a doubling or infinite
        out = np.zeros((self.n, 5), np.uint32)
        for i, x1, y1, x2, y2, inv in zip(live.tolist(), xs, ys, txs, tys, batch_inverse(dx)):  # tr_ref.add, the inversion shared
            lam = (y2 - y1) * inv % P
            out[i] = tr_ref.words5((lam * lam - x1 - x2) % P)
        return out

    @functools.lru_cache(maxsize=None)
    def passes(self, table, filter3):
        """scalar index -> the oracle's filter test of that table's hash, for the words synth_bloom_words(*filter3)"""
        from synth import synth_bloom_words
        return orc.blf_has_many(synth_bloom_words(*filter3), getattr(self, table))

    def records(self, name, first=0, count=None, filter3=None):
        """what mul_batch(K[first : first + count]) reports on the context `name`: one record per selected type for every scalar that has
        a point, through the all-ones filter or - filter3 - through synth_bloom_words(*filter3) as the oracle tests it; key_offset is
        the scalar's index in the call, endo 0"""
        letters = CONTEXTS[name][0]
        count = self.n - first if count is None else count
        assert 0 <= first and first + count <= self.n
        parts = []
        for t in letters:
            sel = self.ok[first:first + count]
            if filter3 is not None:
                sel = sel & self.passes(TABLE[t], filter3)[first:first + count]
            idx = np.nonzero(sel)[0]
            part = np.zeros(len(idx), REC)
            part["key_offset"], part["type"] = idx, TYPE[t]
            part["h160"] = getattr(self, TABLE[t])[first + idx]
            parts.append(part)
        return canon(np.concatenate(parts))


START = 0x6000000123  # the first key of the `add` calls of the tests below


@functools.lru_cache(maxsize=None)
def consecutive(n):
    """the reference over the scalars START ... START + n - 1: what `add` reports for any part of that range, and `mul` for the array
    (tests/test_gpu_regrow.py, tests/test_gpu_call_state.py)"""
    K = np.zeros((n, 4), np.uint64)
    K[:, 0] = np.uint64(START) + np.arange(n, dtype=np.uint64)
    K.setflags(write=False)
    return MulRef(K)


@functools.lru_cache(maxsize=None)
def ref():
    """the reference over shape B's scalars; shape A is its records(name, 0, NA)"""
    return MulRef(scalars()[0])


@functools.lru_cache(maxsize=None)
def plain_ref(n, seed):
    """n seeded random scalars, every one with a point, and their reference: the inputs of the tests of calls past the record cap"""
    K = random_scalars(np.random.default_rng(seed), n)
    r = MulRef(K)
    assert r.ok.all()
    return r
