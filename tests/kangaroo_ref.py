"""The yardstick of `kangaroo` (ECL_PUB | ECL_HERD): a pure-Python restatement, over the oracle's points, of what
ecloop_amd/host/kangaroo_plan.h defines - the SplitMix64 stream, the jump table and the start offsets, the walk with its j + 1 rule, the
record packing, the plan's defaults and limits, and the whole driver with rounds of a given length.  Test infrastructure only."""
import orc

P, N = orc.P, orc.N
M64 = (1 << 64) - 1
TABLE = 32


class Stream:
    def __init__(self, seed):
        self.s = seed & M64

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def draw(self, bits):
        lo = self.next()
        hi = self.next()
        return (lo | hi << 64) & ((1 << bits) - 1)


def table(st, jb):
    s = []
    while len(s) < TABLE:
        v = 1 + st.draw(jb + 1)
        if v not in s:
            s.append(v)
    return s


def distances_and_offsets(seed, herd_log2, jb, sb):
    st = Stream(seed)
    s = table(st, jb)
    return s, [st.draw(sb) for _ in range(1 << herd_log2)]


def add_points(p, q):
    """complete affine addition; None is the point at infinity"""
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % P == 0:
            return None
        lam = 3 * p[0] * p[0] * pow(2 * p[1], P - 2, P) % P
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], P - 2, P) % P
    x = (lam * lam - p[0] - q[0]) % P
    return x, (lam * (p[0] - x) - p[1]) % P


def point_of(k):
    k %= N
    return orc.point_of(k) if k else None


def record(i, d, x):
    """-> (key_offset, (h160 words), endo, compressed) as the library reports a distinguished point"""
    return (d & M64, ((d >> 96) & 0xFFFFFFFF, (d >> 64) & 0xFFFFFFFF, (x >> 224) & 0xFFFFFFFF, (x >> 192) & 0xFFFFFFFF, (x >> 160) & 0xFFFFFFFF),
            i & 1, 6)


def identity_of(rec):
    return rec[1][2] << 64 | rec[1][3] << 32 | rec[1][4]


def distance_of(rec):
    return rec[0] | rec[1][1] << 64 | rec[1][0] << 96


def sort_key(rec):
    return identity_of(rec), distance_of(rec), rec[2]


def start_of(base, q, r, i):
    """the start of kangaroo i with offset r: (base + r) G (tame, i even) or Q + r G (wild, i odd); None is the point at infinity"""
    return add_points(q, point_of(r)) if i & 1 else point_of(base + r)


def jump_of(s, T, pt, d):
    """one jump of one kangaroo standing on pt with distance d, over the distances s and the table points T -> (j, point, distance)"""
    j = (pt[0] >> 32) & 31
    if T[j][0] == pt[0]:
        j = (j + 1) & 31
    return j, add_points(pt, T[j]), d + s[j]


class Herd:
    def __init__(self, base, q, seed, herd_log2, jb, sb):
        self.H = 1 << herd_log2
        self.s, self.r = distances_and_offsets(seed, herd_log2, jb, sb)
        self.T = [orc.point_of(s) for s in self.s]
        self.x, self.y, self.d = [], [], list(self.r)
        for i, r in enumerate(self.r):
            pt = add_points(q, point_of(r)) if i & 1 else point_of(base + r)
            if pt is None:
                raise ValueError("a start is the point at infinity")
            self.x.append(pt[0])
            self.y.append(pt[1])
        self.next_rule = 0  # jumps that took j + 1

    def index_of(self, x):
        j = (x >> 32) & 31
        if self.T[j][0] == x:
            j = (j + 1) & 31
            self.next_rule += 1
        return j

    def step(self, dp):
        """one jump of every kangaroo (Montgomery's trick over the whole herd) -> the records of the distinguished points"""
        H, x, y, d = self.H, self.x, self.y, self.d
        js = [self.index_of(v) for v in x]
        pre, acc = [], 1
        for i in range(H):
            dx = (self.T[js[i]][0] - x[i]) % P
            assert dx, "the shared inversion saw a zero"
            pre.append(acc)
            acc = acc * dx % P
        inv = pow(acc, P - 2, P)
        out, mask = [], (1 << dp) - 1
        for i in range(H - 1, -1, -1):
            tx, ty = self.T[js[i]]
            invk = inv * pre[i] % P
            inv = inv * (tx - x[i]) % P
            lam = (ty - y[i]) * invk % P
            x3 = (lam * lam - x[i] - tx) % P
            y[i] = (lam * (x[i] - x3) - y[i]) % P
            x[i] = x3
            d[i] += self.s[js[i]]
            if d[i] >> 128:
                raise OverflowError("a distance passed 2^128")
            if not x3 & mask:
                out.append(record(i, d[i], x3))
        return out

    def run(self, steps, dp):
        out = []
        for _ in range(steps):
            out += self.step(dp)
        return out


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def plan(a, b, herd_log2=None, dp_bits=None):
    if a < 1 or a > b or b >= N:
        raise ValueError("order")
    wbits = (b - a).bit_length()
    if wbits > 124:
        raise ValueError("width")
    if (herd_log2 is not None and not 1 <= herd_log2 <= 24) or (dp_bits is not None and dp_bits > 32):
        raise ValueError("option")
    half = wbits // 2
    hl = herd_log2 if herd_log2 is not None else clamp(half - 4, 1, 22)
    dp = dp_bits if dp_bits is not None else clamp(max(half - hl - 1, half + 2 - 26), 0, 32)
    return {"wbits": wbits, "herd_log2": hl, "dp": dp, "jb": clamp(half + hl - 2, 4, 120), "sb": clamp(wbits, 1, 124),
            "round_steps": 1 << clamp(min(half - 1 - hl, 34 - hl), 0, 33), "base": a}


def give_up(pl, max_factor):
    return (max_factor << (1 + (pl["wbits"] + 1) // 2)) + (1 << (pl["herd_log2"] + pl["dp"]))


def candidates(base, dt, dw):
    return (base + dt - dw) % N, (-(base + dt) - dw) % N


def search(q, a, b, herd_log2=None, dp_bits=None, seed=0, max_factor=64, round_steps=None, run_round=None):
    """the driver -> (key or None, stats).  run_round(steps, dp) -> records of one round; the default is a Herd of this module"""
    pl = plan(a, b, herd_log2, dp_bits)
    H, dp = 1 << pl["herd_log2"], pl["dp"]
    steps = round_steps or pl["round_steps"]
    if run_round is None:
        run_round = Herd(pl["base"], q, seed, pl["herd_log2"], pl["jb"], pl["sb"]).run
    limit = give_up(pl, max_factor)
    stats = {"jumps": 0, "rounds": 0, "dps": 0, "same_herd": 0, "candidates_checked": 0}
    store = {}
    while True:
        recs = sorted(run_round(steps, dp), key=sort_key)
        stats["jumps"] += steps * H
        stats["rounds"] += 1
        for rec in recs:
            have = store.get(identity_of(rec))
            if have is None:
                store[identity_of(rec)] = rec
                stats["dps"] += 1
            elif have[2] == rec[2]:
                stats["same_herd"] += 1
            else:
                tame, wild = (have, rec) if rec[2] else (rec, have)
                for k in candidates(pl["base"], distance_of(tame), distance_of(wild)):
                    stats["candidates_checked"] += 1
                    if k and orc.point_of(k) == tuple(q):
                        return k, stats
        if stats["jumps"] >= limit:
            return None, stats
