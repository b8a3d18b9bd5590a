#!/usr/bin/env python3
"""bc1p... addresses -> the list lines that `-a t` and `blf-gen -a t` read: the 64 hex digits of each address's output key.

Reads addresses from stdin (one per line, blank lines skipped), writes one 64-digit line per address to stdout.  Refuses - message on
stderr, exit status 1, nothing more written - anything that is not a witness version 1 program of 32 bytes with a valid bech32m checksum
(BIP350): a bc1q... (version 0) address, a bech32 (not -m) checksum, a mistyped character.  Host only, no dependencies.

usage: tools/p2tr_keys.py < addresses.txt > keys.txt"""
import sys

CHARSET = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"
BECH32M = 0x2BC830A3


def polymod(values):
    gen = [0x3B6A57B2, 0x26508E6D, 0x1EA119FA, 0x3D4233DD, 0x2A1462B3]
    chk = 1
    for v in values:
        top = chk >> 25
        chk = (chk & 0x1FFFFFF) << 5 ^ v
        for i in range(5):
            if (top >> i) & 1:
                chk ^= gen[i]
    return chk


def output_key(addr):
    """-> the 32-byte witness program of a P2TR address; ValueError with the reason otherwise"""
    if addr != addr.lower() and addr != addr.upper():
        raise ValueError("mixed case")
    a = addr.lower()
    pos = a.rfind("1")
    if pos < 1 or pos + 7 > len(a) or len(a) > 90:
        raise ValueError("not a bech32 string")
    hrp, rest = a[:pos], a[pos + 1:]
    if any(c not in CHARSET for c in rest):
        raise ValueError("a character outside the bech32 alphabet")
    data = [CHARSET.index(c) for c in rest]
    check = polymod([ord(c) >> 5 for c in hrp] + [0] + [ord(c) & 31 for c in hrp] + data)
    if check == 1:
        raise ValueError("bech32 checksum (witness version 0 encoding), not bech32m")
    if check != BECH32M:
        raise ValueError("bad checksum")
    if data[0] != 1:
        raise ValueError("witness version %d, not 1" % data[0])
    acc, bits, out = 0, 0, bytearray()
    for d in data[1:-6]:
        acc, bits = (acc << 5 | d) & 0xFFF, bits + 5
        if bits >= 8:
            bits -= 8
            out.append(acc >> bits & 0xFF)
    if bits >= 5 or acc & ((1 << bits) - 1):
        raise ValueError("bad padding")
    if len(out) != 32:
        raise ValueError("a %d-byte witness program, not 32" % len(out))
    return bytes(out)


def main():
    for no, line in enumerate(sys.stdin, 1):
        addr = line.strip()
        if not addr:
            continue
        try:
            print(output_key(addr).hex())
        except ValueError as e:
            sys.stderr.write("line %d: %s: %s\n" % (no, addr, e))
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
