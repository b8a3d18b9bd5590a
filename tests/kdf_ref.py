"""The key derivation functions of `mul -raw -kdf`, computed independently of the library, the host program and the engine: the reference
of tests/test_kdf_host.py and tests/test_gpu_kdf.py.

digest(name, line) is pure Python on 64-bit lanes: the sponge of FIPS 202 (rate 136, capacity 512) with the first pad byte as a parameter
- 0x06 gives SHA3-256, which hashlib has, so the permutation, the absorbing and both pad positions can be checked against it (self_check);
0x01 gives the original Keccak-256 of Ethereum; `camp2` is Keccak-256 applied 2031 times (the ethercamp wallet).  digests_many is the same
sponge on numpy arrays over many lines of at most 135 bytes (one block), for the cases with 10^5 ... 10^6 lines."""
import functools
import hashlib

import numpy as np

NAMES = ("sha256", "keccak", "sha3", "camp2")
RATE = 136
CAMP2_HASHES = 2031
M64 = (1 << 64) - 1
# known answers (the issue's; Keccak-256("") is also tests/eth_ref.py's constant)
KNOWN = {
    ("keccak", b""): "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470",
    ("keccak", b"abc"): "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45",
    ("sha3", b"abc"): "3a985da74fe225b2045c172d6bd390bd855f086e3e9d525b46bfe24511431532",
    ("camp2", b""): "26d412aa8b9fea49149a7dbf8b19672d8813f741842ac1847571d335908cbe65",
    ("camp2", b"abc"): "7a44789ed3cd85861c0bbf9693c7e1de1862dd4396c390147ecf1275099c6e6f",
    ("camp2", b"password"): "5e225b381fcf02bd5577885f19b9472234c117dc44df6b59aca6690471dea0a0",
}


def _round_constants():
    """FIPS 202 algorithm 5"""
    out, r = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            if r & 1:
                rc |= 1 << ((1 << j) - 1)
            r <<= 1
            if r & 0x100:
                r ^= 0x171
        out.append(rc)
    return out


def _rotations():
    """FIPS 202 algorithm 2, by flat lane index x + 5y"""
    rot, x, y = [0] * 25, 1, 0
    for t in range(24):
        rot[x + 5 * y] = (t + 1) * (t + 2) // 2 % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rot


RC = _round_constants()
ROT = _rotations()
PI = [(i // 5) + 5 * ((2 * (i % 5) + 3 * (i // 5)) % 5) for i in range(25)]  # lane x + 5y goes to y + 5(2x + 3y)


def keccak_f(a):
    """a: 25 lanes (x + 5y) of 64 bits -> the permuted lanes"""
    for rc in RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ (((c[(x + 1) % 5] << 1) | (c[(x + 1) % 5] >> 63)) & M64) for x in range(5)]
        b = [0] * 25
        for i in range(25):
            v, r = a[i] ^ d[i % 5], ROT[i]
            b[PI[i]] = ((v << r) | (v >> (64 - r))) & M64 if r else v
        a = [b[i] ^ (~b[(i % 5 + 1) % 5 + i - i % 5] & b[(i % 5 + 2) % 5 + i - i % 5]) for i in range(25)]
        a[0] ^= rc
    return a


def sponge256(msg, pad):
    """32 bytes out of the sponge with rate 136 and the first pad byte `pad` (0x01 Keccak-256, 0x06 SHA3-256)"""
    buf = bytearray(msg)
    fill = RATE - len(buf) % RATE
    buf += bytes(fill)
    buf[len(msg)] ^= pad
    buf[-1] ^= 0x80
    a = [0] * 25
    for at in range(0, len(buf), RATE):
        for i in range(RATE // 8):
            a[i] ^= int.from_bytes(buf[at + 8 * i: at + 8 * i + 8], "little")
        a = keccak_f(a)
    return b"".join(v.to_bytes(8, "little") for v in a[:4])


@functools.lru_cache(maxsize=None)
def digest(name, line):
    """the 32-byte digest of `line` (bytes) under -kdf `name`"""
    if name == "sha256":
        return hashlib.sha256(line).digest()
    if name == "sha3":
        return sponge256(line, 0x06)
    if name == "keccak":
        return sponge256(line, 0x01)
    if name == "camp2":
        d = sponge256(line, 0x01)
        for _ in range(CAMP2_HASHES - 1):
            d = sponge256(d, 0x01)
        return d
    raise ValueError(name)


def scalar(name, line):
    """the digest read as a big-endian 256-bit number: the scalar of the line"""
    return int.from_bytes(digest(name, line), "big")


def _keccak_f_many(a):
    """a: (25, n) uint64, permuted in place"""
    u = np.uint64
    for rc in RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ ((c[(x + 1) % 5] << u(1)) | (c[(x + 1) % 5] >> u(63))) for x in range(5)]
        b = [None] * 25
        for i in range(25):
            v, r = a[i] ^ d[i % 5], ROT[i]
            b[PI[i]] = (v << u(r)) | (v >> u(64 - r)) if r else v
        for i in range(25):
            row = i - i % 5
            a[i] = b[i] ^ (~b[(i % 5 + 1) % 5 + row] & b[(i % 5 + 2) % 5 + row])
        a[0] ^= u(rc)


def digests_many(name, text, starts, lengths, chunk=1 << 14):
    """`keccak` / `sha3` of many one-block lines: text = uint8 array, line i = text[starts[i] : starts[i] + lengths[i]], every length
    at most 135 -> (n, 32) uint8 digests.  (In chunks, so that the 25 lane arrays stay in the cache.)"""
    pad = {"keccak": 0x01, "sha3": 0x06}[name]
    starts, lengths = np.asarray(starts, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    assert lengths.max(initial=0) < RATE
    text = np.concatenate([np.asarray(text, dtype=np.uint8), np.zeros(RATE, np.uint8)])
    out = np.zeros((len(starts), 32), np.uint8)
    col = np.arange(RATE, dtype=np.int64)
    for at in range(0, len(starts), chunk):
        s, ln = starts[at: at + chunk], lengths[at: at + chunk]
        blk = text[s[:, None] + col[None, :]]
        blk[col[None, :] >= ln[:, None]] = 0
        blk[np.arange(len(s)), ln] ^= pad
        blk[:, RATE - 1] ^= 0x80
        a = np.zeros((25, len(s)), np.uint64)
        a[:17] = np.ascontiguousarray(blk).view("<u8").T
        _keccak_f_many(a)
        out[at: at + chunk] = np.ascontiguousarray(a[:4].T).astype("<u8").view(np.uint8).reshape(len(s), 32)
    return out


def self_check():
    """sha3 against hashlib at every length that takes another path (around the rate's multiples, both pad bytes in one), the known
    answers, and the numpy form against the pure one"""
    for n in list(range(0, 140)) + [271, 272, 273, 407, 408, 409, 1000]:
        msg = bytes((7 * i + n) & 0xFF for i in range(n))
        if digest("sha3", msg) != hashlib.sha3_256(msg).digest():
            return False
    for (name, line), want in KNOWN.items():
        if digest(name, line).hex() != want:
            return False
    lines = [bytes((i * 31 + j) & 0xFF for j in range(n)) for i, n in enumerate(list(range(0, 136)) + [5, 0, 135])]
    text = np.frombuffer(b"".join(lines), np.uint8)
    lens = np.array([len(l) for l in lines])
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    for name in ("keccak", "sha3"):
        many = digests_many(name, text, starts, lens, chunk=50)
        if [bytes(r) for r in many] != [digest(name, l) for l in lines]:
            return False
    return True
