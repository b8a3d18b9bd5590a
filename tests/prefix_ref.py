"""The yardstick of the prefix search (-p): address text by brute force - base58check with hashlib, bech32 written out from BIP173 - and
"does this value's address start with the pattern", plus the device filter's two-stage test in Python.  It shares no code with the planner
(ecloop_amd/host/prefix_plan.h, engine.prefix_ranges): it never computes a range, it only encodes and compares.  Test infrastructure."""
import bisect
import hashlib
import random

B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
BECH32 = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"
TOP = (1 << 160) - 1


def words5(v):
    return [(v >> (32 * (4 - i))) & 0xFFFFFFFF for i in range(5)]


def value_of(h160):
    v = 0
    for w in h160:
        v = v << 32 | int(w)
    return v


def p2pkh(v):
    """base58check(00 || v as 20 bytes)"""
    raw = b"\x00" + v.to_bytes(20, "big")
    raw += hashlib.sha256(hashlib.sha256(raw).digest()).digest()[:4]
    n, out = int.from_bytes(raw, "big"), ""
    while n:
        n, r = divmod(n, 58)
        out = B58[r] + out
    zeros = 0
    while zeros < len(raw) and raw[zeros] == 0:
        zeros += 1
    return "1" * zeros + out


_POW58 = [58 ** i for i in range(36)]


def p2pkh_head(h20, nchars):
    """the first nchars characters of the P2PKH address of a 20-byte hash with a non-zero first byte - the same base58check, with the
    leading digits taken by one division instead of thirty-four (for tests that encode a million hashes)"""
    assert h20[0] != 0 and 1 <= nchars <= 20
    raw = b"\x00" + h20
    n = int.from_bytes(raw + hashlib.sha256(hashlib.sha256(raw).digest()).digest()[:4], "big")
    d = 34
    while n < _POW58[d - 1]:
        d -= 1
    head, out = n // _POW58[d - (nchars - 1)], ""
    for _ in range(nchars - 1):
        head, r = divmod(head, 58)
        out = B58[r] + out
    return "1" + out


def _polymod(values):
    chk = 1
    for v in values:
        top = chk >> 25
        chk = (chk & 0x1FFFFFF) << 5 ^ v
        for i, g in enumerate((0x3B6A57B2, 0x26508E6D, 0x1EA119FA, 0x3D4233DD, 0x2A1462B3)):
            chk ^= g if (top >> i) & 1 else 0
    return chk


def p2wpkh(v):
    """bech32 of hrp bc, witness version 0 and the 20-byte program (BIP173)"""
    bits = format(v, "0160b")
    data = [0] + [int(bits[i : i + 5], 2) for i in range(0, 160, 5)]
    hrp = [ord(c) >> 5 for c in "bc"] + [0] + [ord(c) & 31 for c in "bc"]
    pm = _polymod(hrp + data + [0] * 6) ^ 1
    return "bc1" + "".join(BECH32[d] for d in data + [(pm >> (5 * (5 - i))) & 31 for i in range(6)])


def eth(v):
    return "0x%040x" % v


def address(pattern, v):
    """the address of the value v in the pattern's form (and, for bech32, its case)"""
    if pattern[:2] in ("0x", "0X"):
        return eth(v)
    if pattern[:4] == "bc1q":
        return p2wpkh(v)
    if pattern[:4] == "BC1Q":
        return p2wpkh(v).upper()
    return p2pkh(v)


def matches(pattern, v):
    a = address(pattern, v)
    return a.startswith(pattern.lower() if pattern[:2] in ("0x", "0X") else pattern)


def b58_decode(s):
    """a base58 string -> its bytes (leading '1's are zero bytes)"""
    n = 0
    for c in s:
        n = n * 58 + B58.index(c)
    body = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return b"\x00" * (len(s) - len(s.lstrip("1"))) + body


def in_table(table, v):
    """table: sorted disjoint (lo, hi) pairs of ints -> v lies inside one (the device's exact stage)"""
    return membership(table)(v)


def membership(table):
    """in_table for many values of one table"""
    los = [lo for lo, _ in table]

    def inside(v):
        i = bisect.bisect_right(los, v)
        return i > 0 and v <= table[i - 1][1]
    return inside


def stage1(table, v, bucket_bits=24):
    """the device's stage 1: some range intersects v's bucket"""
    s = 160 - bucket_bits
    i = bisect.bisect_right([lo >> s for lo, _ in table], v >> s)  # the last range that starts in or before the bucket ends last
    return i > 0 and table[i - 1][1] >> s >= v >> s


# ---- the device filter's questions: tables and values for prefix.h on the host and ecl_hip_diag_bloom on the GPU (the same ones)

def expect(pairs, values):
    los, s = [lo for lo, _ in pairs], 160 - 24
    blos = [lo >> s for lo in los]
    want_s1, want = [], []
    for v in values:
        i = bisect.bisect_right(los, v)
        want.append(int(i > 0 and v <= pairs[i - 1][1]))
        j = bisect.bisect_right(blos, v >> s)
        want_s1.append(int(j > 0 and pairs[j - 1][1] >> s >= v >> s))
    return want_s1, want


def random_table(rng, n, widths):
    """n sorted disjoint ranges: random starts, widths drawn from `widths` (bits), clipped so that none reaches the next"""
    starts = sorted({rng.getrandbits(160) for _ in range(n)})
    out = []
    for i, lo in enumerate(starts):
        room = (starts[i + 1] if i + 1 < len(starts) else TOP + 1) - lo - 1
        out.append((lo, lo + min(room, rng.getrandbits(rng.choice(widths)))))
    return out


def boundary_values(pairs, rng, extra=2000):
    vals = {0, TOP}
    for lo, hi in [pairs[0], pairs[-1]] + rng.sample(pairs, min(len(pairs), 3000)):
        vals |= {lo, hi, max(lo - 1, 0), min(hi + 1, TOP), (lo + hi) // 2}
    vals |= {rng.getrandbits(160) for _ in range(extra)}
    for lo, hi in rng.sample(pairs, min(len(pairs), 200)):  # same bucket as a range, outside it: stage 1 passes, the exact stage decides
        vals |= {max(lo - rng.getrandbits(100), 0), min(hi + rng.getrandbits(100), TOP)}
    return sorted(vals)


def prefix_filter_cases():
    """name -> (ranges, values): shared with the GPU test, which asks ecl_hip_diag_bloom the same questions"""
    rng = random.Random(2024)
    cases = {}
    for n, widths in ((1, (0, 40, 150)), (2, (0, 1)), (300, (0, 1, 8, 32, 33, 64, 100, 130, 140)), (1 << 16, (0, 5, 60, 120, 139))):
        pairs = random_table(rng, n, widths)
        cases["random%d" % n] = (pairs, boundary_values(pairs, rng, 3000 if n < 1000 else 20000))
    base = rng.getrandbits(128) << 32
    word4 = [(base + 10, base + 20), (base + 21, base + 21), (base + 23, base + 0xFFFFFFF0), (base + 0xFFFFFFF2, base + 0xFFFFFFFF)]  # differ in word 4 only
    cases["word4"] = (word4, sorted({base + d for d in (0, 9, 10, 11, 20, 21, 22, 23, 24, 0xFFFFFFF0, 0xFFFFFFF1, 0xFFFFFFF2, 0xFFFFFFFF)} | {base - 1, base + (1 << 32)}))
    single = sorted({rng.getrandbits(160) for _ in range(500)} | {0, TOP})
    cases["single"] = ([(v, v) for v in single], sorted({w for v in single for w in (v - 1, v, v + 1) if 0 <= w <= TOP}))
    cases["whole"] = ([(0, TOP)], [0, 1, TOP - 1, TOP] + [rng.getrandbits(160) for _ in range(100)])
    cases["ends"] = ([(0, 0), (TOP, TOP)], [0, 1, 2, TOP - 2, TOP - 1, TOP, 1 << 136, (1 << 136) - 1])
    edge = 0xABCDEF << 136  # the first value of bucket 0xabcdef
    straddle = [(edge - 5, edge + 5), (edge + (1 << 136) - 1, edge + (1 << 136)), (edge + (5 << 136) - 1, edge + (9 << 136) + 3)]
    cases["straddle"] = (straddle, sorted({e + d for e in (edge, edge + (1 << 136), edge + (5 << 136), edge + (9 << 136), edge + (2 << 136), edge + (10 << 136), edge - (1 << 136))
                                           for d in (-6, -5, -2, -1, 0, 1, 3, 4, 5, 6, 1 << 135)}))
    adjacent = [(1000, 1999), (2000, 2999), (3000, 3000), (3001, 1 << 150), ((1 << 150) + 1, (1 << 150) + 1)]
    cases["adjacent"] = (adjacent, [999, 1000, 1999, 2000, 2999, 3000, 3001, 3002, (1 << 150) - 1, 1 << 150, (1 << 150) + 1, (1 << 150) + 2])
    return cases
