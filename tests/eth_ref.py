"""The Ethereum address of a public key computed independently of the library for the ETH tests: a pure-Python Keccak-f[1600] sponge
written from FIPS 202 with the first pad byte as a parameter - 0x06 gives SHA-3 (which hashlib has, so the permutation and the sponge
can be checked), 0x01 the original Keccak that Ethereum uses."""
import hashlib

import numpy as np

M64 = (1 << 64) - 1
RHO = [[0, 36, 3, 41, 18], [1, 44, 10, 45, 2], [62, 6, 43, 15, 61], [28, 55, 25, 21, 56], [27, 20, 39, 8, 14]]  # [x][y]


def _round_constants():
    """FIPS 202 algorithm 5: the bits of RC[i] from the LFSR x^8 + x^6 + x^5 + x^4 + 1"""
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


RC = _round_constants()


def rotl(v, n):
    n %= 64
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


def keccak_f(a):
    """a[x][y]: 25 lanes of 64 bits, permuted in place"""
    for rnd in range(24):
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x - 1) % 5] ^ rotl(c[(x + 1) % 5], 1) for x in range(5)]
        b = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = rotl(a[x][y] ^ d[x], RHO[x][y])
        for x in range(5):
            for y in range(5):
                a[x][y] = b[x][y] ^ (~b[(x + 1) % 5][y] & M64 & b[(x + 2) % 5][y])
        a[0][0] ^= RC[rnd]


def keccak256(msg, pad=0x01):
    """the 32-byte digest of the sponge with rate 136 and capacity 512; pad: the first padding byte (0x01 Keccak, 0x06 SHA-3)"""
    rate = 136
    m = bytearray(msg)
    m.append(pad)
    m.extend(b"\0" * (-len(m) % rate))
    m[-1] |= 0x80
    a = [[0] * 5 for _ in range(5)]
    for at in range(0, len(m), rate):
        for i in range(rate // 8):
            a[i % 5][i // 5] ^= int.from_bytes(m[at + 8 * i:at + 8 * i + 8], "little")
        keccak_f(a)
    return b"".join(a[i % 5][i // 5].to_bytes(8, "little") for i in range(4))


def eth_address(x, y):
    """the 20 address bytes of the public key (x, y)"""
    return keccak256(x.to_bytes(32, "big") + y.to_bytes(32, "big"))[12:]


def eth_hex(x, y):
    return eth_address(x, y).hex()


def eth_words(x, y):
    """the address in h160_t words (word k = bytes 4k..4k+3, big-endian)"""
    d = eth_address(x, y)
    return [int.from_bytes(d[4 * k:4 * k + 4], "big") for k in range(5)]


def keccak_many(msgs):
    """Keccak-256 (pad 0x01, rate 136) of n messages of 64 bytes, (n, 64) uint8 -> (n, 32) uint8: keccak_f over arrays, in pieces that
    stay in cache"""
    n = len(msgs)
    out = np.zeros((n, 4), np.uint64)
    lanes = np.ascontiguousarray(msgs).view("<u8").reshape(n, 8)
    for at in range(0, n, 1 << 14):
        blk = lanes[at:at + (1 << 14)]
        m = len(blk)
        a = [[np.zeros(m, np.uint64) for _ in range(5)] for _ in range(5)]
        for i in range(8):
            a[i % 5][i // 5] = blk[:, i].copy()
        a[8 % 5][8 // 5] = np.full(m, 0x01, np.uint64)
        a[16 % 5][16 // 5] = np.full(m, 0x80 << 56, np.uint64)

        def rotl(v, r):  # (of arrays: shadows the module's rotl of integers)
            r %= 64
            return (v << np.uint64(r)) | (v >> np.uint64(64 - r)) if r else v
        for rnd in range(24):
            c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
            d = [c[(x - 1) % 5] ^ rotl(c[(x + 1) % 5], 1) for x in range(5)]
            b = [[None] * 5 for _ in range(5)]
            for x in range(5):
                for y in range(5):
                    b[y][(2 * x + 3 * y) % 5] = rotl(a[x][y] ^ d[x], RHO[x][y])
            for x in range(5):
                for y in range(5):
                    a[x][y] = b[x][y] ^ (~b[(x + 1) % 5][y] & b[(x + 2) % 5][y])
            a[0][0] = a[0][0] ^ np.uint64(RC[rnd])
        for i in range(4):
            out[at:at + m, i] = a[i % 5][i // 5]
    return out.view(np.uint8).reshape(n, 32)


def self_check(lengths=range(0, 273, 7)):
    """the sponge with pad 0x06 is hashlib's SHA3-256; Keccak-256 of the empty message is the well-known constant"""
    for n in lengths:
        msg = bytes((i * 131 + n) & 0xFF for i in range(n))
        assert keccak256(msg, 0x06) == hashlib.sha3_256(msg).digest(), n
    assert keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    return True
