"""The yardstick of the `brain` tests: a template's candidates by itertools.product, written apart from engine.py's divmod, the host
program's division and the device's odometer.  A template is `positions`: a list of positions, each a list of alternatives (bytes).
Candidate i is the i-th element of the product in its own order - the last position runs fastest."""
import itertools
import struct


def count(positions):
    t = 1
    for p in positions:
        t *= len(p)
    return t


def candidates(positions, first=0, n=None):
    """candidates first ... first + n - 1 (n = None: to the end), by walking the product from its start: small indices only"""
    stop = None if n is None else first + n
    return [b"".join(c) for c in itertools.islice(itertools.product(*positions), first, stop)]


def candidate(positions, i):
    """candidate i of a template of any size: the product of the one-element slices that the mixed-radix digits of i choose - the digits
    are taken from the most significant end, by the weights prod_{q > p} c_q"""
    weights = [count(positions[p + 1:]) for p in range(len(positions))]
    picked = []
    for p, w in zip(positions, weights):
        d, i = i // w, i % w
        picked.append(p[d:d + 1])
    (c,) = itertools.product(*picked)
    return b"".join(c)


def window(positions, first, n):
    """candidates first ... first + n - 1 of a template of any size"""
    return [candidate(positions, first + j) for j in range(n)]


def blob(positions):
    """the packed template of include/ecloop_hip.h (ECL_GEN), with struct"""
    pool, alts, pos, first = b"", [], [], 0
    for p in positions:
        pos.append(struct.pack("<II", len(p), first))
        first += len(p)
        for a in p:
            alts.append(struct.pack("<II", len(pool), len(a)))
            pool += a
    return struct.pack("<4sB3xII", b"GEN\0", len(positions), first, len(pool)) + b"".join(pos) + b"".join(alts) + pool
