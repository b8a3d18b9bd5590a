"""The yardstick of the zero-digit tests: the signed window recoding of `mul`'s table (csrc/mul_kernels.h: wtab_recode) restated on Python
integers, and what follows from it for the window sum (wtab_sum_fast): which scalars hold a digit of magnitude 0 - they take a stand-in
table point there and are summed again out of line by the complete formulas - and in which window, by which cause.

A scalar t < 2^256 is cut into ceil(256 / W) windows of W bits (the last one is as narrow as what is left).  Window w's value is
v = raw + carry, the carry coming from the window below; where v > 2^(W-1) the digit is v - 2^W (a negated table point) and 1 is carried
into the next window - except in the last window, whose carry would have nowhere to go and whose row holds every value.  A digit is zero
in two ways: raw = 0 without a carry ("raw0"), or raw = 2^W - 1 with one ("carry": v = 2^W, the digit 2^W - 2^W).

Shares nothing with the code under test; pinned to hand-worked values in tests/test_digit_ref.py."""

WIDTHS = (8, 11, 13, 22, 26)  # the widths the zero-digit tests run at


def windows(W):
    return -(-256 // W)


def signed_digits(t, W):
    """the digits d_w with t = sum d_w 2^(W w), and the carry each window received -> [(d_w, carry into w)]"""
    assert 0 <= t < 1 << 256 and 8 <= W <= 29
    out, carry, n = [], 0, windows(W)
    for w in range(n):
        v = ((t >> (W * w)) & ((1 << W) - 1)) + carry
        neg = w + 1 < n and v > 1 << (W - 1)
        out.append((v - (1 << W) if neg else v, carry))
        carry = 1 if neg else 0
    return out


def zero_digits(t, W):
    """-> [(window, "raw0" | "carry")] for every digit of t of magnitude zero, lowest window first"""
    return [(w, "carry" if carry else "raw0") for w, (d, carry) in enumerate(signed_digits(t, W)) if d == 0]


def window_class(w, W):
    """where wtab_sum_fast meets window w: 0 and 1 are its affine + affine start, 2 is fetched ahead of the loop, the last one ("top") is
    the row that is not recoded, the others ("middle") come from the loop's own look-ahead"""
    assert 0 <= w < windows(W)
    return "top" if w == windows(W) - 1 else ("w0", "w1", "w2")[w] if w < 3 else "middle"


CLASSES = ("w0", "w1", "w2", "middle", "top")


def windows_walked(wave, W):
    """wtab_sum_fast's wave-uniform loop bound for the scalars of one wave: windows in which no lane has a bit (nor a carry to come) are
    cut off the top, never below two windows; a zero digit at or above the bound is not flagged"""
    nw, bits = windows(W), max(t.bit_length() for t in wave)
    while nw > 2 and bits < (nw - 1) * W:
        nw -= 1
    return nw


def flagged(t, wave, W):
    """the zero digits of t that wtab_sum_fast flags when t runs in a wave with the scalars `wave` (t among them): those below the
    wave's bound.  Non-empty: t is summed again by the complete formulas"""
    nw = windows_walked(wave, W)
    return [(w, cause) for w, cause in zero_digits(t, W) if w < nw]
