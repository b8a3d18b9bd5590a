"""The yardstick of the `seed` tests: BIP39 phrase -> seed -> BIP32 path -> private key, from hashlib.pbkdf2_hmac, hmac and a few lines of
affine secp256k1 arithmetic.  Nothing here is shared with the product (ecloop_amd.engine.bip39_key is the product's own mirror);
tests/test_seed_host.py pins this file to the published BIP39 / BIP32 vectors."""
import functools
import hashlib
import hmac

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
HARD = 1 << 31
PHRASE_A = b"abandon " * 11 + b"about"


def _add(a, b):
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
    acc, q = None, G
    while k:
        if k & 1:
            acc = _add(acc, q)
        q = _add(q, q)
        k >>= 1
    return acc


def ser_p(k):
    x, y = mul_g(k)
    return bytes([2 | (y & 1)]) + x.to_bytes(32, "big")


@functools.lru_cache(maxsize=None)
def seed_of(phrase, passphrase=b"", rounds=2048):
    return hashlib.pbkdf2_hmac("sha512", phrase, b"mnemonic" + passphrase, rounds, 64)


def master_of(seed):
    """-> (k, c), k = 0 for an invalid node"""
    I = hmac.new(b"Bitcoin seed", seed, hashlib.sha512).digest()
    k = int.from_bytes(I[:32], "big")
    return (k if 0 < k < N else 0), I[32:]


def child_of(I, k):
    """BIP32's rule on an HMAC result -> (k', c') or None"""
    il = int.from_bytes(I[:32], "big")
    if il >= N or (il + k) % N == 0:
        return None
    return (il + k) % N, I[32:]


def ckd(k, c, index, ser=ser_p):
    """CKDpriv -> (k', c') or None for an invalid child; ser: k -> serP(k G) (a caller with a faster k G than mul_g's passes its own)"""
    data = (b"\0" + k.to_bytes(32, "big") if index & HARD else ser(k)) + index.to_bytes(4, "big")
    return child_of(hmac.new(c, data, hashlib.sha512).digest(), k)


def walk(k, c, path, ser=ser_p):
    for index in path:
        if k == 0:
            return 0
        nxt = ckd(k, c, index, ser)
        if nxt is None:
            return 0
        k, c = nxt
    return k


def key_of_seed(seed, path, ser=ser_p):
    k, c = master_of(seed)
    return walk(k, c, path, ser)


def key_of(phrase, path, passphrase=b"", ser=ser_p):
    """the private key (int; 0 for an invalid node) of `path` (a list of 32-bit elements, bit 31 = hardened)"""
    return key_of_seed(seed_of(phrase, passphrase), path, ser)


def path_of(text):
    """m/44'/0'/0'/0/0 -> [44 | HARD, HARD, HARD, 0, 0]"""
    parts = text.split("/")
    assert parts[0] == "m"
    return [int(p.rstrip("'h")) | (HARD if p[-1] in "'h" else 0) for p in parts[1:]]
