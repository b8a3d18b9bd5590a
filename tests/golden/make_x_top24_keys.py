#!/usr/bin/env python3
"""Find private keys whose public key's x - or its image beta x, beta^2 x under the endomorphism - has 24 leading one bits: the keys at
which emit33_xwords (csrc/emit33.h) takes its exact block, 2^-24 per key and image.

    python tests/golden/make_x_top24_keys.py [first key] [groups] [processes]

A plain batched walk on Python integers, nothing else: groups of 1025 consecutive keys around a centre C = c G, the members C +- i G
(i = 1 ... 512) by the affine addition with ONE inversion per group (Montgomery's trick over the 512 differences and the step to the next
centre), x alone, three values per key.  Three to four times 10^5 keys per second and process; the default range, 50 000 groups from
0x40000000 (51.25 M keys), takes about three minutes on one.  Output: tests/golden/x_top24_keys.json, rows {"key", "image" (the power of beta),
"x" (the image's x)}.  tests/test_digit_ref.py re-derives every row from the oracle's points."""
import json
import multiprocessing
import os
import sys

P = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFFC2F
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
HALF = 512
GROUP = 2 * HALF + 1
TOP = (1 << 256) - (1 << 232)  # x >= TOP: 24 leading one bits
FIRST, GROUPS = 0x40000000, 50000
HERE = os.path.dirname(os.path.abspath(__file__))


def add(a, b):
    if a is None or b is None:
        return a or b
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def mul_g(k):
    acc, q = None, (GX, GY)
    while k:
        if k & 1:
            acc = add(acc, q)
        q = add(q, q)
        k >>= 1
    return acc


def table():
    """i G for i = 1 ... HALF, and the step GROUP G"""
    out, q = [], None
    for _ in range(HALF):
        q = add(q, (GX, GY))
        out.append(q)
    return out, mul_g(GROUP)


def walk(job):
    """groups g0 ... g0 + n - 1 of the walk that starts at key `first` -> [(key, image)]"""
    first, g0, n = job
    tab, (jx, jy) = table()
    c = first + g0 * GROUP + HALF
    cx, cy = mul_g(c)
    hits = []

    def look(x, key):
        for image in range(3):
            if x >= TOP:
                hits.append((key, image))
            x = x * BETA % P

    for _ in range(n):
        pre, acc = [], 1
        for gx, _ in tab:
            pre.append(acc)
            acc = acc * (gx - cx) % P
        inv = pow(acc * (jx - cx) % P, -1, P)
        invj = inv * acc % P  # 1 / (jx - cx)
        inv = inv * (jx - cx) % P
        look(cx, c)
        for i in range(HALF - 1, -1, -1):
            gx, gy = tab[i]
            invk = inv * pre[i] % P
            inv = inv * (gx - cx) % P
            s = -cx - gx
            lam = (gy - cy) * invk % P
            look((lam * lam + s) % P, c + i + 1)
            lam = (gy + cy) * invk % P
            look((lam * lam + s) % P, c - i - 1)
        lam = (jy - cy) * invj % P
        nx = (lam * lam - cx - jx) % P
        cx, cy = nx, (lam * (cx - nx) - cy) % P
        c += GROUP
    return hits


def main():
    first = int(sys.argv[1], 0) if len(sys.argv) > 1 else FIRST
    groups = int(sys.argv[2]) if len(sys.argv) > 2 else GROUPS
    procs = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    per = 500
    jobs = [(first, g, min(per, groups - g)) for g in range(0, groups, per)]
    if procs > 1:
        with multiprocessing.Pool(procs) as pool:
            parts = pool.map(walk, jobs)
    else:
        parts = [walk(j) for j in jobs]
    rows = []
    for key, image in sorted(h for part in parts for h in part):
        x = mul_g(key)[0] * pow(BETA, image, P) % P
        assert x >= TOP
        rows.append({"key": key, "image": image, "x": "%064x" % x})
    print("%d keys from 0x%x: %s" % (groups * GROUP, first, [sum(r["image"] == i for r in rows) for i in range(3)]))
    with open(os.path.join(HERE, "x_top24_keys.json"), "w") as f:
        json.dump({"first": first, "keys": groups * GROUP, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
