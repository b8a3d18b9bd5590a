"""Raw-limb cases at the limits of fe256.h's magnitude contract, and their reference in Python integers.

One generator with a fixed seed, used unchanged by the CPU test (tests/test_devsrc_host.py, through dh_limb_op) and by the GPU test
(tests/test_gpu_primitives.py, through Device.diag_limbs): both run csrc/limb_ops.h's limb_op on the same (n, 6, 9) uint32 arrays.

A limb's ceiling for magnitude m and excess s is m * 2^29 + s (limb 8: m * 2^24 + s); s = m * E, with E the bound fe256.h derives for
limb 2 of a product, so a lazy sum of m products is inside the test.  Magnitude 0 stands for "normalised limbs" (below 2^29 / 2^24, no
excess) where a function's comment asks for a normalised operand.  The reference: value(limbs) = sum n[i] 2^(29 i) as a Python integer;
field results are compared mod p, point steps with their polynomial formulas mod p (the inputs are no curve points), canonical results bit
for bit, and every raw result against the magnitude its function documents."""
import os
import random
import re

import numpy as np

P = 2**256 - 2**32 - 977
E = 449  # fe256.h, "Magnitude discipline": limb 2 of a product is at most 2^29 - 1 + E
SEED = 0x29A9
B29, B24 = 1 << 29, 1 << 24
P_LIMBS = [0x1FFFFC2F, 0x1FFFFFF7] + [0x1FFFFFFF] * 6 + [0xFFFFFF]
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
N_FIELD, N_INV, N_POINT = 20000, 4000, 10000

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the operation numbers: read from the one place they are written
OP = {k: int(v) for k, v in re.findall(r"\b(LIMB_[A-Z0-9_]+) = (\d+)", open(os.path.join(ROOT, "ecloop_amd", "csrc", "limb_ops.h")).read())}
LIMB_IN, LIMB_OUT = 6, 4

MUL_PAIRS = [(1, 7), (7, 1), (2, 3), (3, 2), (1, 6), (1, 4), (3, 1), (1, 3), (2, 2), (1, 1)]  # fe_mul: m1 * m2 <= 7
# (name of the family's operation, input magnitudes by input slot (None: unused, zero), cases).  The magnitudes are those the headers document:
FAMILIES = (
    [("LIMB_MUL", pr, N_FIELD) for pr in MUL_PAIRS]                                              # fe_mul: m1 * m2 <= 7
    + [("LIMB_SQR", (m,), N_FIELD) for m in (1, 2)]                                              # fe_sqr: m <= 2
    + [("LIMB_MUL2", MUL_PAIRS[i] + MUL_PAIRS[(i + 3) % 10], N_FIELD) for i in range(10)]        # fe_mul2: two fe_mul
    + [("LIMB_SQR2", pr, N_FIELD) for pr in ((1, 1), (1, 2), (2, 1), (2, 2))]                    # fe_sqr2: two fe_sqr
    + [(op, (m,), N_FIELD) for op in ("LIMB_WEAK", "LIMB_NORM", "LIMB_PARITY", "LIMB_IS_ZERO") for m in range(1, 8)]  # limbs below 2^32: m <= 7
    + [(("LIMB_NEG1", m), (m,), N_FIELD) for m in range(1, 7)]                                   # fe_neg(a, m): a of magnitude <= m; op LIMB_NEG1 + m - 1
    + [("LIMB_INV_DIVSTEPS", (m,), N_INV) for m in range(1, 8)]                                  # "any magnitude <= 7 in"
    + [("LIMB_INV_FERMAT", (m,), N_INV) for m in (1, 2)]                                         # "Input magnitude <= 2"
    # X, Y, ZZ, ZZZ, qx, qy: "X, ZZ, ZZZ in / out 1, Y in / out <= 3"; the table point's coordinates enter 1 x 1 products
    + [("LIMB_XYZZ_MADD", (1, 3, 1, 1, 1, 1), N_POINT), ("LIMB_XYZZ_MADD_NEG", (1, 3, 1, 1, 1, 1), N_POINT)]
    + [("LIMB_XYZZ_MMADD", (1, 1, None, None, 1, 1), N_POINT)]                                   # affine + affine: fe_sub wants magnitude 1
    # "set-up code keeps every value at magnitude 1"
    + [(op, (1, 1, 1, None, 1, 1), N_POINT) for op in ("LIMB_JAC_MADD", "LIMB_JAC_MADD_NEG", "LIMB_JAC_MADD_DBL")]
    + [("LIMB_JAC_DBL", (1, 1, 1), N_POINT)]
    # X, Y, gx, gy, invk: "gy: the table's y (normalised), Y: magnitude 1"; X + gx is negated as magnitude 2; invk is a product
    + [("LIMB_PUB_PAIR_X", (1, 1, 1, 0, 1), N_POINT)]
    + [("LIMB_PUB_ENDO_X", (m,), N_POINT) for m in range(1, 5)]                                  # "x: magnitude <= 4"
    + [("LIMB_PUB_WORDS20", (m,), N_POINT) for m in range(1, 7)]                                 # "x: magnitude <= 6"
)
WEAK_TARGET_OPS = ("LIMB_WEAK", "LIMB_NORM", "LIMB_PARITY", "LIMB_IS_ZERO")


def op_of(name):
    return OP[name[0]] + name[1] - 1 if isinstance(name, tuple) else OP[name]


def label(name, mags):
    return "%s%s" % (name if isinstance(name, str) else "LIMB_NEG%d" % name[1], tuple(mags))


def limbs_of(v):
    """the 9 x 29 digits of 0 <= v < 2^256 (the canonical limb form when v < p)"""
    return [(v >> (29 * i)) & (B29 - 1) for i in range(8)] + [v >> 232]


def values(a):
    """(n, 9) limbs -> object array of Python integers: sum n[i] 2^(29 i)"""
    o = np.asarray(a).astype(object)
    v = o[:, 8]
    for i in range(7, -1, -1):
        v = v * B29 + o[:, i]
    return v


def ceiling(m, s):
    if m == 0:
        return [B29 - 1] * 8 + [B24 - 1]
    return [m * B29 + s] * 8 + [m * B24 + s]


def special_table(m):
    """limb forms inside magnitude m: k p, k p +- 1, 2, 976, 977 for k = 0 .. 7, the canonical values around p - 1, p, p + 1 and 2^256 - 1"""
    rows = []
    for k in range(8):
        base = [k * x for x in P_LIMBS]
        rows.append(base)
        for d in (1, 2, 976, 977):
            rows.append([base[0] + d] + base[1:])
            if k:
                rows.append([base[0] - d] + base[1:])
    rows += [limbs_of(v) for v in (0, 1, 2, P - 2, P - 1, P, P + 1, P + 2, 2**256 - 2, 2**256 - 1, 2**256 - 2**32 - 1, 2**256 - 2**32)]
    c = ceiling(m, 0)
    rows = [r for r in rows if all(x <= y for x, y in zip(r, c))]
    return np.array(rows, dtype=np.int64)


def weak_target(rnd, m, c, bit24):
    """limbs of magnitude m (ceilings c) whose weakly normalised value lands in [2^256, 2p) - limb 8 comes out with bit 24 set - or in
    [p, 2^256) with it clear: the two ways into fe_normalize's final subtraction"""
    x = rnd.randrange(m)  # what fe_normalize_weak folds: n[8] >> 24
    if bit24:
        w = 2**256 + rnd.choice([0, 1, 2, 976, 977, 2**32 + 976, 2**32 + 977, rnd.randrange(2**33), rnd.randrange(2**29)])
    else:
        w = P + rnd.choice([0, 1, 2, 976, 977, 2**32 + 975, 2**32 + 976, rnd.randrange(2**32 + 977), rnd.randrange(2**29)])
    v = w + x * P
    n = limbs_of(v)
    over = n[8] - ((x + 1) * B24 - 1)
    if over > 0:  # the overflow must come out of the carry pass, not out of the fold
        n[8] -= over
        n[7] += over << 29
    for i in range(8, 0, -1):  # a random redundant form of the same integer
        room = (c[i - 1] - n[i - 1]) >> 29
        r = rnd.randint(0, max(0, min(n[i] - (x * B24 if i == 8 else 0), room)))
        n[i] -= r
        n[i - 1] += r << 29
    assert n[8] >> 24 == x and all(0 <= a <= b for a, b in zip(n, c)) and sum(a << (29 * i) for i, a in enumerate(n)) == v
    assert (w >= 2**256) == bool(bit24) and P <= w < 2 * P
    return n


def element(rs, rnd, m, n, weak_targets=False):
    """n elements of magnitude m: (n, 9) int64, every limb in [0, ceiling]"""
    s = np.where(rs.randint(0, 4, n) == 0, 0, m * E).astype(np.int64)  # three in four carry the excess
    c = np.array(ceiling(m, 0), dtype=np.int64)[None, :] + (s[:, None] if m else np.zeros((n, 1), dtype=np.int64))
    tab = special_table(m)
    pat = rs.randint(0, 8 if weak_targets else 7, n)
    pat[0] = 0
    out = np.zeros((n, 9), dtype=np.int64)
    for p in range(7):
        idx = np.nonzero(pat == p)[0]
        k = len(idx)
        cc = c[idx]
        if p == 0:    # every limb at the ceiling
            v = cc
        elif p == 1:  # each limb 0 or the ceiling
            v = cc * rs.randint(0, 2, (k, 9))
        elif p == 2:  # the ceiling minus 0 .. 3
            v = cc - rs.randint(0, 4, (k, 9))
        elif p == 3:  # uniform in [0, ceiling]
            v = np.minimum((rs.random_sample((k, 9)) * (cc + 1)).astype(np.int64), cc)
        elif p == 4:  # a mix of the values at which a carry or a mask changes
            opts = np.stack([np.zeros_like(cc), np.ones_like(cc), cc, cc - 1, cc // 2, np.full_like(cc, B29 - 1), np.full_like(cc, B29)])
            pick = rs.randint(0, 7, (k, 9))
            v = np.minimum(np.take_along_axis(opts, pick[None], 0)[0], cc)
        elif p == 5:  # multiples of p's own limbs
            mm = max(m, 1)
            opts = np.array([mm * P_LIMBS[0], mm * P_LIMBS[1], mm * P_LIMBS[2]], dtype=np.int64)
            v = opts[rs.randint(0, 3, (k, 9))]
            v[:, 8] = mm * P_LIMBS[8]
        else:         # k p +- d and the canonical edge values
            v = tab[rs.randint(0, len(tab), k)]
        out[idx] = v
    if weak_targets:
        for i in np.nonzero(pat == 7)[0]:
            out[i] = weak_target(rnd, m, [int(x) for x in c[i]], rnd.randrange(2))
    assert (out >= 0).all() and (out <= c).all() and (out < 2**32).all()
    return out, tab


def families(only=None):
    """-> (name, op number, magnitudes, cases (n, 6, 9) uint32, left_out, cases moved in or out) for every family (only: of one
    operation), each from its own fixed seed"""
    moved = {}
    for fi, (name, mags, n) in enumerate(FAMILIES):
        rs = np.random.RandomState([SEED, fi])
        rnd = random.Random(SEED * 1000 + fi)
        base = base_of(name)
        if only is not None and base != only and not (base == "LIMB_JAC_MADD" and only.startswith("LIMB_JAC_MADD")):
            continue
        cases = np.zeros((n, LIMB_IN, 9), dtype=np.int64)
        single = sum(m is not None for m in mags) == 1
        for slot, m in enumerate(mags):
            if m is None:
                continue
            el, tab = element(rs, rnd, m, n, weak_targets=base in WEAK_TARGET_OPS)
            if single:  # one operand: the whole table of special forms, one by one
                k = min(len(tab), n - 1)
                el[1 : 1 + k] = tab[:k]
            cases[:, slot] = el
        left_out = 0
        if base.startswith("LIMB_JAC_MADD"):
            x, y, z, qx, qy = (values(cases[:, s]) for s in (0, 1, 2, 4, 5))
            u2, s2 = qx * z * z % P, qy * z * z * z % P
            if base == "LIMB_JAC_MADD":
                # the generic branch.  Cases that happen to have h = 0 are not dropped: they go through the two exceptional-branch
                # families below (by rr), so no case is left out
                h0 = np.asarray((u2 - x) % P == 0, dtype=bool)
                rr0 = np.asarray((s2 - y) % P == 0, dtype=bool)
                moved = {"LIMB_JAC_MADD_NEG": cases[h0 & ~rr0], "LIMB_JAC_MADD_DBL": cases[h0 & rr0]}
                left_out = int(h0.sum()) - sum(len(v) for v in moved.values())
                cases = cases[~h0]
            else:  # X (and Y) rebuilt so that h = 0 (and rr = 0): the canonical limbs of qx Z^2 (qy Z^3)
                for i in range(n):
                    cases[i, 0] = limbs_of(int(u2[i]))
                    if base == "LIMB_JAC_MADD_DBL":
                        cases[i, 1] = limbs_of(int(s2[i]))
                    elif (int(s2[i]) - int(y[i])) % P == 0:  # (a Y that happens to equal qy Z^3: off by one)
                        cases[i, 1] = limbs_of((int(s2[i]) + 1) % P)
                cases = np.concatenate([cases, moved[base]])
        if only is None or base == only:
            yield name, op_of(name), mags, cases.astype(np.uint32), left_out, len(cases) - n


# ---------------------------------------------------------------------------------------------------------------- the reference

class Mismatch(AssertionError):
    pass


def _fail(what, fam, i, cases, out, flag):
    raise Mismatch("%s: %s, case %d\n in  = %s\n out = %s\n flag = %d" % (fam, what, i, cases[i].tolist(), out[i].tolist(), int(flag[i])))


def _all(cond, what, fam, cases, out, flag):
    cond = np.asarray(cond, dtype=bool)
    if not cond.all():
        _fail(what, fam, int(np.nonzero(~cond)[0][0]), cases, out, flag)


def _mag(a, m, limb2_excess=0, top=None):
    """every limb inside magnitude m: below m 2^29 (limb 2: + limb2_excess), limb 8 at most `top` (default m 2^24 - 1)"""
    a = a.astype(np.int64)
    lim = np.array([m * B29 - 1] * 8 + [m * B24 - 1 if top is None else top], dtype=np.int64)
    lim[2] += limb2_excess
    return (a <= lim[None, :]).all(axis=1)


def _product(a):  # what fe_mul / fe_sqr return: magnitude 1, limb 2 up to 2^29 - 1 + E
    return _mag(a, 1, E)


def _weak(a):  # what fe_normalize_weak returns: limbs below 2^29, limb 8 below 2^24 plus the pass's carry (at most 7), value below 2 p
    return _mag(a, 1, 0, top=B24 + 6) & (values(a) < 2 * P)


def _words(v):
    return np.array([[(int(x) >> (32 * j)) & 0xFFFFFFFF for j in range(8)] + [0] for x in v], dtype=np.uint32)


def _canon(v):
    return np.array([limbs_of(int(x)) for x in v], dtype=np.uint32)


def _inv(v):
    return np.array([pow(int(x), -1, P) if x else 0 for x in v], dtype=object)  # (0 -> 0, like both inversions)


def _madd(x, y, zz, zzz, qx, qy, neg):
    u2, s2 = qx * zz % P, qy * zzz % P
    if neg:
        s2 = -s2 % P
    h, r = (u2 - x) % P, (s2 - y) % P
    hh = h * h % P
    hhh = hh * h % P
    x3 = (r * r - hhh - 2 * x * hh) % P
    return x3, (r * (x * hh - x3) - y * hhh) % P, h, hh, hhh


def _dbl(x, y, z):
    a, b = x * x % P, y * y % P
    c = b * b % P
    d = 2 * ((x + b) ** 2 - a - c) % P
    e = 3 * a % P
    x3 = (e * e - 2 * d) % P
    return x3, (e * (d - x3) - 8 * c) % P, 2 * y * z % P


def check(name, mags, cases, out, flag):
    """compares one family's results with the reference; -> the largest amount by which limb 2 of a product exceeded 2^29 - 1 (or None)"""
    base = name[0] if isinstance(name, tuple) else name
    fam = label(name, mags)
    n = len(cases)
    assert out.shape == (n, LIMB_OUT, 9) and flag.shape == (n,)
    ok = lambda cond, what: _all(cond, what, fam, cases, out, flag)
    vin = [values(cases[:, s]) for s in range(LIMB_IN)]
    vout = [values(out[:, s]) % P for s in range(LIMB_OUT)]
    zero = lambda *slots: ok(np.all([(out[:, s] == 0).all(axis=1) for s in slots], axis=0), "unused outputs are not zero")
    products = []
    if base in ("LIMB_MUL", "LIMB_SQR"):
        want = vin[0] * (vin[1] if base == "LIMB_MUL" else vin[0]) % P
        ok(vout[0] == want, "value"), zero(1, 2, 3)
        products = [0]
    elif base in ("LIMB_MUL2", "LIMB_SQR2"):
        w0, w1 = (vin[0] * vin[1] % P, vin[2] * vin[3] % P) if base == "LIMB_MUL2" else (vin[0] * vin[0] % P, vin[1] * vin[1] % P)
        ok(vout[0] == w0, "first value"), ok(vout[1] == w1, "second value"), zero(2, 3)
        products = [0, 1]
    elif base == "LIMB_WEAK":
        ok(vout[0] == vin[0] % P, "value"), ok(_weak(out[:, 0]), "not weakly normalised"), zero(1, 2, 3)
    elif base == "LIMB_NORM":
        r = vin[0] % P
        ok((out[:, 0] == _canon(r)).all(axis=1), "not the canonical limbs"), ok((out[:, 1] == _words(r)).all(axis=1), "words"), zero(2, 3)
    elif base == "LIMB_PARITY":
        ok(flag == np.array([int(x) & 1 for x in vin[0] % P], dtype=np.uint32), "parity"), zero(0, 1, 2, 3)
    elif base == "LIMB_IS_ZERO":
        ok(flag == np.array([int(x == 0) for x in vin[0] % P], dtype=np.uint32), "is_zero"), zero(0, 1, 2, 3)
    elif base == "LIMB_NEG1":
        m = mags[0]
        ok(values(out[:, 0]) == (m + 1) * P - vin[0], "not (m + 1) p - a as an integer"), ok(_mag(out[:, 0], m + 1), "magnitude"), zero(1, 2, 3)
    elif base in ("LIMB_INV_DIVSTEPS", "LIMB_INV_FERMAT"):
        r = _inv(vin[0] % P)
        if base == "LIMB_INV_DIVSTEPS":
            ok((out[:, 0] == _canon(r)).all(axis=1), "not the canonical limbs of the inverse")
        else:
            ok(vout[0] == r, "value")
            products = [0]
        ok((out[:, 1] == _words(r)).all(axis=1), "words"), zero(2, 3)
    elif base in ("LIMB_XYZZ_MADD", "LIMB_XYZZ_MADD_NEG", "LIMB_XYZZ_MMADD"):
        x, y, qx, qy = vin[0], vin[1], vin[4], vin[5]
        zz, zzz = (1, 1) if base == "LIMB_XYZZ_MMADD" else (vin[2], vin[3])
        x3, y3, h, hh, hhh = _madd(x, y, zz, zzz, qx, qy, base == "LIMB_XYZZ_MADD_NEG")
        ok(vout[0] == x3, "X3"), ok(vout[1] == y3, "Y3"), ok(vout[2] == zz * hh % P, "ZZ3"), ok(vout[3] == zzz * hhh % P, "ZZZ3"), ok(flag == 0, "inf")
        ok(_weak(out[:, 0]), "X3 not weakly normalised"), ok(_mag(out[:, 1], 3, E, top=3 * B24), "Y3 above magnitude 3")
        products = [2, 3]
    elif base in ("LIMB_JAC_MADD", "LIMB_JAC_MADD_NEG", "LIMB_JAC_MADD_DBL", "LIMB_JAC_DBL"):
        x, y, z, qx, qy = vin[0], vin[1], vin[2], vin[4], vin[5]
        zero(3)
        if base == "LIMB_JAC_MADD_NEG":  # P = -Q: the point comes back as it is, flagged infinite
            ok(flag == 1, "inf"), ok((out[:, :3] == cases[:, :3]).all(axis=(1, 2)), "the point changed")
        else:
            if base == "LIMB_JAC_MADD":
                x3, y3, h, hh, hhh = _madd(x, y, z * z % P, z * z * z % P, qx, qy, False)
                z3 = z * h % P
                products = [2]
            else:
                x3, y3, z3 = _dbl(x, y, z)
                ok(_weak(out[:, 2]), "Z3 not weakly normalised")
            ok(vout[0] == x3, "X3"), ok(vout[1] == y3, "Y3"), ok(vout[2] == z3, "Z3"), ok(flag == 0, "inf")
            ok(_weak(out[:, 0]), "X3 not weakly normalised"), ok(_weak(out[:, 1]), "Y3 not weakly normalised")
    elif base == "LIMB_PUB_PAIR_X":
        x, y, gx, gy, invk = vin[:5]
        for s, sign in ((0, 1), (1, -1)):
            lam = (sign * gy - y) * invk % P
            ok(vout[s] == (lam * lam - x - gx) % P, "x of C %s G" % "+-"[s]), ok(_mag(out[:, s], 4, E, top=4 * B24), "above magnitude 4")
        zero(2, 3)
    elif base == "LIMB_PUB_ENDO_X":
        bx = BETA * vin[0] % P
        ok(vout[0] == bx, "beta x"), ok(vout[1] == (-vin[0] - bx) % P, "beta^2 x"), ok(_mag(out[:, 1], 6, 0, top=6 * B24), "above magnitude 6"), zero(2, 3)
        products = [0]
    elif base == "LIMB_PUB_WORDS20":
        want = np.array([[(int(v) >> (32 * (7 - j))) & 0xFFFFFFFF for j in range(5)] + [0] * 4 for v in vin[0] % P], dtype=np.uint32)
        ok((out[:, 0] == want).all(axis=1), "leading words"), zero(1, 2, 3)
    else:
        raise AssertionError("no reference for " + fam)
    worst = None
    for s in products:
        worst = max(worst or 0, int(out[:, s, 2].astype(np.int64).max()) - (B29 - 1))
    for s in products:
        ok(_product(out[:, s]), "a product above magnitude 1 (limb 2 exceeds 2^29 - 1 by up to %d, the bound is %d)" % (worst, E))
    return worst


def base_of(name):
    return name[0] if isinstance(name, tuple) else name


BASES = sorted({base_of(f[0]) for f in FAMILIES}, key=lambda b: OP[b])  # the operations, one test case each (LIMB_NEG1: fe_neg for m = 1 .. 6)


def run(call, base):
    """every family of one operation through call(op, cases) -> (out, flag) and the reference; fe_mul2 / fe_sqr2 also against two fe_mul /
    fe_sqr limb for limb.  -> {"cases" run, "planned" (the families' sizes), "moved" (jac_madd cases with h = 0 that came in from (+) or
    went out of (-) the generic family: cases = planned + moved), "left_out" (cases that ran nowhere), "limb2_excess": the largest excess of a product's
    limb 2 over 2^29 - 1 (None: the operation returns no product), "family": where it was seen}"""
    total = left = moved = 0
    worst, where = None, None
    for name, op, mags, cases, left_out, delta in families(base):
        out, flag = call(op, cases)
        try:
            w = check(name, mags, cases, out, flag)
        except Mismatch as e:
            raise Mismatch("%s\n(largest excess of limb 2 over 2^29 - 1 seen before: %s in %s; bound %d)" % (e, worst, where, E)) from None
        if name in ("LIMB_MUL2", "LIMB_SQR2"):
            single = OP["LIMB_MUL"] if name == "LIMB_MUL2" else OP["LIMB_SQR"]
            for s in range(2):
                one = np.zeros_like(cases)
                if name == "LIMB_MUL2":
                    one[:, :2] = cases[:, 2 * s : 2 * s + 2]
                else:
                    one[:, 0] = cases[:, s]
                o1, _ = call(single, one)
                _all((o1[:, 0] == out[:, s]).all(axis=1), "result %d differs from the single operation's limbs" % s, label(name, mags), cases, out, flag)
        if w is not None and (worst is None or w > worst):
            worst, where = w, label(name, mags)
        total += len(cases)
        left += left_out
        moved += delta
    planned = sum(f[2] for f in FAMILIES if base_of(f[0]) == base)
    return {"cases": total, "planned": planned, "moved": moved, "left_out": left, "limb2_excess": worst, "family": where}
