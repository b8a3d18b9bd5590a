"""What every `add` search type must report for a range of keys, computed once and shared: the reference of tests/test_gpu_walk_steps.py.

For the keys start ... start + nkeys - 1 and their six endomorphism images a WalkRef holds the 20 bytes a record of each type carries:
addr33 / addr65 from ONE oracle call over the covering 2048-key groups (orc.add_range, all-ones filter, -a cu -endo), mapped back to
(offset, image) through calc_priv; P2SH by tests/p2sh_ref.py over the addr33 hashes; Ethereum by eth_ref.keccak_many over the oracle's
points (orc.point_of) and their images (x times beta, y negated), a fixed sample of it re-derived with the pure-Python eth_ref.eth_words
from the point of calc_priv's key; Taproot by tests/tr_ref.py.  Each table is built when a context first asks for it.

records() gives a context's expectation for a call as a sorted numpy array, canon() brings the device's records into the same form,
difference() compares the two.  A filter is applied with the oracle's own test (OrcFilter.check), once per table.  CPU only: checked
against tests/fake_device.py and the known answers of the P2SH / Ethereum / Taproot tests in tests/test_walk_ref.py."""
import functools

import numpy as np

import eth_ref
import orc
import p2sh_ref
import tr_ref
from ecloop_amd.engine import LAMBDA, calc_priv

P, N = orc.P, orc.N
GROUP = 2048  # the oracle hashes whole groups of this many keys
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE  # (x, y) -> (BETA x, y) is the point map of k -> LAMBDA k
TYPE = {"c": 1, "u": 0, "s": 2, "e": 3, "t": 4}  # a record's `compressed` field
TABLE = {"c": "h33", "u": "h65", "s": "p2sh", "e": "eth", "t": "tr"}
REC = np.dtype([("key_offset", "<u8"), ("endo", "u1"), ("type", "u1"), ("h160", "<u4", (5,))])
ORC_FOUND = np.dtype([("h160", "<u4", (5,)), ("compressed", "u1"), ("endo", "u1"), ("pad", "u1", (2,)), ("pk", "<u8", (4,))])
assert ORC_FOUND.itemsize == orc.C.sizeof(orc.Found)


def _contexts():
    """the 17: name -> (type letters, endo, keyword arguments of capi.Device)"""
    out = {}
    for letters in ("c", "u", "cu", "s", "cs", "us", "cus"):
        for endo in (False, True):
            out[letters + ("-endo" if endo else "")] = (letters, endo, dict(a33="c" in letters, a65="u" in letters, p2sh="s" in letters, endo=endo))
    out["e"] = ("e", False, dict(a33=False, eth=True))
    out["e-endo"] = ("e", True, dict(a33=False, eth=True, endo=True))
    out["t"] = ("t", False, dict(a33=False, tr=True))
    return out


CONTEXTS = _contexts()
# half group B, lanes T, start, nkeys: lane 2's first centre start + B + 2 * 2B is the jump point's scalar T * 2B, the call has four rounds,
# the fourth with nkeys mod (T * 2B) live keys in lane 0 alone
SHAPES = {"A": (8, 256, 4056, 3 * 4096 + 5), "B": (2, 256, 1014, 3 * 1024 + 3)}
FILTER3 = (3, 33, "a|b")  # synth.synth_bloom_words: three words (no power of two) of bit density 0.75


def centre(start, B, T, lane, rnd=0):
    """the scalar of the centre of a lane's group in a round (add_walk.inc: base = (rnd * T + lane) * 2B, the centre is base + B)"""
    return start + (rnd * T + lane) * 2 * B + B


def group_offsets(B, T, lane, rnd):
    """the key offsets a lane hashes in a round"""
    base = (rnd * T + lane) * 2 * B
    return range(base, base + 2 * B)


def canon(recs):
    """records (capi.FOUND_DTYPE or REC) -> REC sorted by (key_offset, endo, type)"""
    out = np.zeros(len(recs), REC)
    out["key_offset"], out["endo"], out["h160"] = recs["key_offset"], recs["endo"], recs["h160"]
    out["type"] = recs["type"] if "type" in recs.dtype.names else recs["compressed"]
    return out[np.lexsort((out["type"], out["endo"], out["key_offset"]))]


def difference(got, want):
    """"" when two canon() arrays are the same records, else where they part"""
    if len(got) == len(want) and np.array_equal(got, want):
        return ""
    n = min(len(got), len(want))
    bad = np.nonzero(got[:n] != want[:n])[0]
    at = int(bad[0]) if len(bad) else n
    row = lambda a: "(off %d, endo %d, type %d, %s)" % (a[at]["key_offset"], a[at]["endo"], a[at]["type"], orc.hex160(a[at]["h160"])) if at < len(a) else "nothing"
    return "%d records, %d expected, %d differ in the common part; first at %d: got %s, expected %s" % (len(got), len(want), len(bad), at, row(got), row(want))


class WalkRef:
    def __init__(self, start, nkeys, near=0):
        """near: a key offset whose 32 neighbours [near - 8, near + 24) join the Ethereum sample"""
        assert 0 < start and start + GROUP * ((nkeys + GROUP - 1) // GROUP) < N
        self.start, self.nkeys, self.near = start, nkeys, near

    @functools.cached_property
    def btc(self):
        """(h33, h65): (nkeys, 6, 5) uint32 each, [offset, image] -> the oracle's hash"""
        span = GROUP * ((self.nkeys + GROUP - 1) // GROUP)
        rc, out, n, _, hashed = orc.add_range(orc.OrcFilter(bloom_words=ONES), self.start, self.start + span, a33=True, a65=True, endo=True,
                                              verify=False, threads=4, cap=12 * span)
        assert rc == 0 and hashed == span and n == 12 * span
        found = np.frombuffer(out, ORC_FOUND, n)
        slot = {calc_priv(self.start, 1, off, e): 6 * off + e for off in range(span) for e in range(6)}
        pk = found["pk"].tobytes()
        idx = np.array([slot[int.from_bytes(pk[32 * i:32 * i + 32], "little") % N] for i in range(n)], np.int64)
        assert np.array_equal(idx % 6, found["endo"])
        tables = []
        for comp in (1, 0):
            sel = found["compressed"] == comp
            assert np.array_equal(np.bincount(idx[sel], minlength=6 * span), np.ones(6 * span, np.int64))  # every key x image once
            t = np.zeros((6 * span, 5), np.uint32)
            t[idx[sel]] = found["h160"][sel]
            tables.append(t.reshape(span, 6, 5)[: self.nkeys].copy())
        return tuple(tables)

    @functools.cached_property
    def h33(self):
        return self.btc[0]

    @functools.cached_property
    def h65(self):
        return self.btc[1]

    @functools.cached_property
    def p2sh(self):
        return np.array([[p2sh_ref.p2sh_of_h33(h) for h in row] for row in self.h33], np.uint32).reshape(self.nkeys, 6, 5)

    @functools.cached_property
    def eth(self):
        pts = [orc.point_of(self.start + off) for off in range(self.nkeys)]
        msgs = b"".join((x * pow(BETA, e // 2, P) % P).to_bytes(32, "big") + ((P - y) if e & 1 else y).to_bytes(32, "big") for x, y in pts for e in range(6))
        digest = eth_ref.keccak_many(np.frombuffer(msgs, np.uint8).reshape(-1, 64))
        words = np.ascontiguousarray(digest[:, 12:]).view(">u4").astype(np.uint32).reshape(self.nkeys, 6, 5)
        sample = {(i // 6, i % 6) for i in range(0, 6 * self.nkeys, 97)}
        sample |= {(off, e) for off in range(max(0, self.near - 8), min(self.nkeys, self.near + 24)) for e in range(6)}
        for off, e in sorted(sample):  # the pure-Python sponge over the point of the image's own key: the arrays, beta and the image order
            assert eth_ref.eth_words(*orc.point_of(calc_priv(self.start, 1, off, e))) == [int(w) for w in words[off, e]], (off, e)
        return words

    @functools.cached_property
    def tr(self):
        keys = [tr_ref.output_key(self.start + off) for off in range(self.nkeys)]
        assert None not in keys  # (a tweak >= n: one key in 2^128)
        return np.array([tr_ref.words5(q) for q in keys], np.uint32).reshape(self.nkeys, 1, 5)

    @functools.lru_cache(maxsize=None)
    def passes(self, table, filter3):
        """[offset, image] -> the oracle's filter test of that hash, for the words synth_bloom_words(*filter3)"""
        from synth import synth_bloom_words
        flt = orc.OrcFilter(bloom_words=synth_bloom_words(*filter3))
        t = getattr(self, table)
        return np.array([flt.check(h) for h in t.reshape(-1, 5).tolist()], bool).reshape(t.shape[:2])

    def records(self, name, first=0, count=None, filter3=None):
        """what add_range(start + first, count) reports on the context `name`: every key x image x selected type once, through the all-ones
        filter or - filter3 - through synth_bloom_words(*filter3) as the oracle tests it; key_offset counts from the call's own start"""
        letters, endo, _ = CONTEXTS[name]
        count = self.nkeys - first if count is None else count
        assert 0 <= first and first + count <= self.nkeys
        imgs = 6 if endo else 1
        parts = []
        for t in letters:
            part = np.zeros(count * imgs, REC)
            part["key_offset"] = np.repeat(np.arange(count, dtype=np.uint64), imgs)
            part["endo"] = np.tile(np.arange(imgs, dtype=np.uint8), count)
            part["type"] = TYPE[t]
            part["h160"] = getattr(self, TABLE[t])[first:first + count, :imgs].reshape(-1, 5)
            if filter3 is not None:
                part = part[self.passes(TABLE[t], filter3)[first:first + count, :imgs].reshape(-1)]
            parts.append(part)
        return canon(np.concatenate(parts))


@functools.lru_cache(maxsize=None)
def ref_of(shape):
    B, T, start, nkeys = SHAPES[shape]
    assert centre(start, B, T, 2) == T * 2 * B  # lane 2 starts on the jump point: its step to the next centre is the tangent
    return WalkRef(start, nkeys, near=group_offsets(B, T, 2, 1)[0])
