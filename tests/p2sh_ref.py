"""The P2SH-P2WPKH hash (BIP49 "3..." addresses) computed independently of the library for the P2SH tests: hashlib's SHA-256 and the
oracle's RIPEMD-160 block (orc_rmd160_block, oracle/orc.c) - hashlib here has no ripemd160."""
import hashlib
import struct

import orc


def ripemd160(data):
    """RIPEMD-160 of a message shorter than 56 bytes (one block) -> the 20-byte digest"""
    assert len(data) < 56
    block = data + b"\x80" + b"\0" * (55 - len(data)) + struct.pack("<Q", 8 * len(data))
    x = (orc.C.c_uint32 * 16)(*struct.unpack("<16I", block))
    out = (orc.C.c_uint32 * 5)()
    orc.lib().orc_rmd160_block(out, x)
    return struct.pack("<5I", *out)


def hash160(data):
    return ripemd160(hashlib.sha256(data).digest())


def words(digest):
    """20 digest bytes -> h160_t words (word k = bytes 4k..4k+3, big-endian)"""
    return list(struct.unpack(">5I", digest))


def p2sh_of_h33(h33):
    """h160_t words of a compressed key's hash160 -> h160_t words of hash160(0x00 0x14 || it)"""
    return words(hash160(b"\x00\x14" + struct.pack(">5I", *[int(w) for w in h33])))


def p2sh_hex(h33_hex):
    return hash160(b"\x00\x14" + bytes.fromhex(h33_hex)).hex()
