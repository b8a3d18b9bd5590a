#!/usr/bin/env python3
"""Find curve points whose Taproot tweak holds a zero signed digit at the production widths of `mul`'s table (22 and 26 bits): the points
at which k_tr_check (csrc/tr_kernels.h) sends a key through tr_sum_complete.  The tweak is a SHA-256 output, so such points are found,
not made: ecl_hip_diag_tr takes any affine point, and x need not come from a known key.

    python tests/golden/make_tr_zero_digit_points.py [processes]

hashlib and Python integers only.  The walk takes x = 2, 3, ...; hashes t = taptweak(x); keeps x where t has a zero digit
(tests/digit_ref.py; before that a cheap filter for a window of all zeros or all ones) and x^3 + 7 is a square; and stops for a width
once it holds, in the order met, one x for each class of digit_ref.CLASSES - window 0, window 1, window 2, a middle window, the top
window - and one whose digit was made by a carry.  The rows alternate between the two roots y, so that both lifts occur.  A class of the
26-bit table turns up once in about 2^27 values of x: minutes of CPU on a few processes.  Output: tests/golden/tr_zero_digit_points.json,
rows {"W", "window", "cause", "x", "y"}; tests/test_digit_ref.py re-checks every row."""
import hashlib
import json
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import digit_ref  # noqa: E402

P = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFFC2F
TAG = hashlib.sha256(b"TapTweak").digest()
M256 = (1 << 256) - 1
CHUNK = 1 << 22
WANTED = digit_ref.CLASSES + ("carry",)


def scan(job):
    """x in [x0, x1) whose tweak has a zero digit at width W -> [(x, t)]"""
    W, x0, x1 = job
    n = digit_ref.windows(W)
    lo = sum(1 << (W * w) for w in range(n))  # bit 0 of every window
    hi = sum(1 << (min(W * w + W, 256) - 1) for w in range(n))  # its highest bit
    head = hashlib.sha256(TAG + TAG)
    out = []
    for x in range(x0, x1):
        h = head.copy()
        h.update(x.to_bytes(32, "big"))
        t = int.from_bytes(h.digest(), "big")
        u = t ^ M256
        if ((t - lo) & u & hi) or ((u - lo) & t & hi):  # some window is 0, or some window is all ones
            if digit_ref.zero_digits(t, W):
                out.append((x, t))
    return out


def root(x):
    """y with y^2 = x^3 + 7, or None"""
    c = (x * x * x + 7) % P
    y = pow(c, (P + 1) // 4, P)
    return y if y * y % P == c else None


def search(W, pool, procs):
    have, rows, x0 = {}, [], 2
    while len(have) < len(WANTED):
        jobs = [(W, x0 + i * CHUNK, x0 + (i + 1) * CHUNK) for i in range(procs)]
        x0 += len(jobs) * CHUNK
        for part in pool.map(scan, jobs):
            for x, t in part:
                digits = digit_ref.zero_digits(t, W)
                new = [(digit_ref.window_class(w, W), w, cause) for w, cause in digits if digit_ref.window_class(w, W) not in have]
                new += [("carry", w, cause) for w, cause in digits if cause == "carry" and "carry" not in have][:1]
                if not new or len(have) == len(WANTED):
                    continue
                y = root(x)
                if y is None:
                    continue
                for name, w, cause in new:
                    have.setdefault(name, x)
                y = y if len(rows) % 2 == 0 else P - y
                rows.append({"W": W, "window": new[0][1], "cause": new[0][2], "x": "%064x" % x, "y": "%064x" % y})
        print("W = %d: x < %d, %s" % (W, x0, sorted(have)), flush=True)
    return rows


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    with multiprocessing.Pool(procs) as pool:
        rows = [r for W in (22, 26) for r in search(W, pool, procs)]
    with open(os.path.join(HERE, "tr_zero_digit_points.json"), "w") as f:
        json.dump({"rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
