"""The yardstick of the masked Ethereum patterns (-p 0xdead*beef): "does this address match the pattern" by a regular expression over the
lower-case text, the mask filter's test in Python integers, the synthetic cases both the g++ build of csrc/mask.h and the device answer, and
a stand-in device for engine.prefix_search.  It shares no code with the planner (ecloop_amd/host/mask_plan.h, engine.mask_table): it never
computes a mask from a pattern, it only writes the address out and compares text.  Test infrastructure."""
import functools
import re

import numpy as np

TOP = (1 << 160) - 1
FULL = TOP


def words5(v):
    return [(v >> (32 * (4 - i))) & 0xFFFFFFFF for i in range(5)]


def value_of(h160):
    v = 0
    for w in h160:
        v = v << 32 | int(w)
    return v


def eth(v):
    return "0x%040x" % v


def regex_of(pattern):
    """? -> one hex digit, * -> any run of them; the end is anchored only when * is present (a pattern without one is a prefix)"""
    assert pattern[:2] in ("0x", "0X")
    body = "".join("[0-9a-f]" if c == "?" else "[0-9a-f]*" if c == "*" else re.escape(c.lower()) for c in pattern[2:])
    return re.compile("0x" + body + ("$" if "*" in pattern else ""))


def matches(pattern, v):
    return regex_of(pattern).match(eth(v)) is not None


def first_match(patterns, v):
    return next((i for i, p in enumerate(patterns) if matches(p, v)), None)


def has(entries, v):
    """entries: (mask, value) pairs of 160-bit integers"""
    return any((v ^ val) & m == 0 for m, val in entries)


def table_of(entries):
    return np.array([words5(m) + words5(v) for m, v in entries], np.uint32).reshape(-1, 10)


def entries_of(table):
    return [(value_of(r[:5]), value_of(r[5:])) for r in np.asarray(table)]


def mask_filter_cases():
    """name -> (entries, values): for each of the five words an entry whose only fixed bits lie in that word, with the value that hits
    and the same value with each fixed bit flipped; the two bits at each word boundary; an all-zero mask; sixteen entries of which only the
    last one matches"""
    base = 0x0123456789ABCDEFDEADBEEF0BADF00DFEEDFACE
    cases = {}
    for w in range(5):
        m = 0x00FFFF00 << (32 * (4 - w))
        cases["word%d" % w] = ([(m, base & m)], [base, base ^ (TOP & ~m)] + [base ^ (1 << b) for b in range(32 * (4 - w), 32 * (5 - w))])
    for w in range(4):
        lo = 32 * (4 - w)  # bit lo is the lowest of word w, bit lo - 1 the highest of word w + 1
        m = 3 << (lo - 1)
        cases["boundary%d" % w] = ([(m, base & m)], [base, base ^ (1 << lo), base ^ (1 << (lo - 1)), base ^ (TOP & ~m)])
    cases["zero_mask"] = ([(0, 0)], [0, base, TOP])
    cases["last_of_16"] = ([(FULL, base ^ (i + 1)) for i in range(15)] + [(FULL, base)], [base, base ^ 16, base ^ (1 << 159)] + [base ^ (i + 1) for i in range(15)])
    return cases


def expect(entries, values):
    return [int(has(entries, v)) for v in values]


@functools.lru_cache(maxsize=None)
def eth_words_of(x, y):
    """the address words of the point (x, y) by tests/eth_ref.py, kept: the tests and the stand-in device ask for the same points"""
    import eth_ref
    return tuple(int(w) for w in eth_ref.eth_words(x, y))


class FakeMaskDevice:
    """Same surface as capi.Device(eth=True, mask=True[, origin=True]) as far as engine.KeySearch uses it, no GPU: the keys' addresses by
    the pure-Python Keccak of tests/eth_ref.py over the oracle's points, the mask test above in place of the device's"""
    tables = []
    opened = []

    def __init__(self, device=0, a33=True, a65=False, endo=False, ord_offs=0, eth=False, mask=False, origin=False):
        assert eth and mask and not a33 and not a65
        self.endo, self.offs, self.origin, self.entries = endo, ord_offs, origin, None
        FakeMaskDevice.opened.append(dict(endo=endo, origin=origin))

    def close(self):
        pass

    def set_bloom(self, words):
        raise AssertionError("a mask search sets a mask table, not a bloom filter")

    set_prefixes = set_bloom

    def set_masks(self, table):
        table = np.asarray(table)
        assert table.dtype == np.uint32 and table.ndim == 2 and table.shape[1] == 10 and 1 <= len(table) <= 16
        FakeMaskDevice.tables.append(table.copy())
        self.entries = entries_of(table)

    def set_list(self, hashes):
        raise AssertionError("a mask context has no list")

    def set_geometry(self, half_group=0, max_lanes=0):
        pass

    def geometry(self):
        return 64, 512

    def _point(self, k, origin):
        import orc
        return orc.point_of(k) if origin is None else _add(origin, orc.point_of(k))

    def add_range(self, start, nkeys, cap=4096, origin=None):
        from ecloop_amd import capi, engine
        assert (origin is not None) == bool(self.origin)
        recs = []
        for off in range(nkeys):
            x, y = self._point((start + (off << self.offs)) % engine.N, origin)
            for e in range(6 if self.endo else 1):
                ex, ey = engine.splitkey_image_origin((x, y), e)
                h = list(eth_words_of(ex, ey))
                if has(self.entries, value_of(h)):
                    recs.append((off, h, e))
        arr = np.zeros(len(recs), dtype=capi.FOUND_DTYPE)
        for j, (off, h, e) in enumerate(recs):
            arr[j]["key_offset"], arr[j]["h160"], arr[j]["endo"], arr[j]["compressed"] = off, h, e, 3
        self.kept = arr
        return arr[:cap].copy(), len(arr)

    def fetch_found(self, first, n):
        return self.kept[first:first + n].copy()

    def verify_eth(self, ks, origin=None):
        pts = [self._point(k, None if origin is None else origin[i]) for i, k in enumerate(ks)]
        return np.array([eth_words_of(x, y) for x, y in pts], np.uint32).reshape(-1, 5), np.ones(len(ks), np.uint8)


def _add(p, q):
    """affine addition on secp256k1 (p != +-q or p == q)"""
    P = 2**256 - 2**32 - 977
    (x1, y1), (x2, y2) = p, q
    lam = (3 * x1 * x1) * pow(2 * y1, -1, P) % P if p == q else (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P
