"""The yardstick of the Taproot tests: BIP341 / BIP86 key-path output keys restated in pure Python - hashlib's SHA-256, Python integers,
affine secp256k1 arithmetic written here, public keys from the oracle (orc.point_of).  Shares nothing with the code under test.  Pinned
in tests/test_tr_host.py to the published BIP341 wallet vector and to three private-key known answers."""
import hashlib

import orc

P, N = orc.P, orc.N
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
TAG = hashlib.sha256(b"TapTweak").digest()


def add(a, b):
    """affine addition, None = the point at infinity"""
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def mul_g(k):
    """k G by double-and-add (any k >= 0)"""
    acc, q = None, (GX, GY)
    while k:
        if k & 1:
            acc = add(acc, q)
        q = add(q, q)
        k >>= 1
    return acc


def tweak(x):
    """t = int(SHA-256(T || T || x)), T = SHA-256("TapTweak"): the tagged hash of BIP340 over the x-only key, no merkle root (BIP86)"""
    return int.from_bytes(hashlib.sha256(TAG + TAG + x.to_bytes(32, "big")).digest(), "big")


def lift(x, y):
    """the point with this x and even y"""
    return (x, y) if y % 2 == 0 else (x, P - y)


def output_key_of_point(x, y):
    """Q.x of Q = lift(P) + t G, or None where BIP341 gives none (t >= n, or Q at infinity)"""
    t = tweak(x)
    if t >= N:
        return None
    q = add(lift(x, y), orc.point_of(t) if t else None)  # (t G from the oracle, like P; mul_g above is the slow cross-check of both)
    return None if q is None else q[0]


def output_key(k):
    """the output key of the private key k (None for k = 0 mod n)"""
    if k % N == 0:
        return None
    return output_key_of_point(*orc.point_of(k % N))


def words8(q):
    """32 bytes as eight big-endian words (the h160_t convention continued)"""
    return [(q >> (32 * (7 - i))) & 0xFFFFFFFF for i in range(8)]


def words5(q):
    """the leading 20 bytes: what a filter, a list and a found record hold"""
    return words8(q)[:5]


# ---- bech32m (BIP350), for the addresses of the known answers
CHARSET = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"


def _polymod(values):
    gen = [0x3B6A57B2, 0x26508E6D, 0x1EA119FA, 0x3D4233DD, 0x2A1462B3]
    chk = 1
    for v in values:
        b = chk >> 25
        chk = (chk & 0x1FFFFFF) << 5 ^ v
        for i in range(5):
            chk ^= gen[i] if (b >> i) & 1 else 0
    return chk


def p2tr_address(q, hrp="bc"):
    data = [1]
    acc, bits = 0, 0
    for byte in q.to_bytes(32, "big"):
        acc, bits = acc << 8 | byte, bits + 8
        while bits >= 5:
            bits -= 5
            data.append(acc >> bits & 31)
    if bits:
        data.append(acc << (5 - bits) & 31)
    exp = [ord(c) >> 5 for c in hrp] + [0] + [ord(c) & 31 for c in hrp]
    pm = _polymod(exp + data + [0] * 6) ^ 0x2BC830A3
    return hrp + "1" + "".join(CHARSET[d] for d in data + [pm >> 5 * (5 - i) & 31 for i in range(6)])
