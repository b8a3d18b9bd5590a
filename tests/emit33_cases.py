"""Operand sets and their reference for csrc/emit33.h (the addr33-only emit path of the add kernels), shared by the CPU test
(tests/test_emit33_host.py, through csrc/tools/emit33_host.cpp) and the GPU test (tests/test_gpu_emit33.py, through Device.diag_limbs).

The operands are tests/limb_cases.py's: x at magnitudes 1 .. 4 beside y at 1 .. 3, every pattern of `element` at the magnitude ceilings,
its weak-pass targets (values fe_normalize_weak leaves in [p, 2p), with and without bit 24 in limb 8) and its table of k p +- d and
canonical edge values in both slots, so y == 0, 1, p - 1 are there.  The reference is the oracle's hash160 of (x mod p, y mod p), the
parity of y mod p and bloom.h's index of probe 0 in Python integers; it is computed once and shared."""
import functools
import random

import numpy as np

import limb_cases
import orc

N_PER_PAIR = 2000


@functools.lru_cache(maxsize=None)
def _sets():
    parts = []
    half = N_PER_PAIR // 2
    for mx in range(1, 5):
        for my in range(1, 4):
            rs = np.random.RandomState([limb_cases.SEED, 33, mx, my])
            rnd = random.Random(limb_cases.SEED * 1000 + 33 * 16 + mx * 4 + my)
            x, tabx = limb_cases.element(rs, rnd, mx, N_PER_PAIR, weak_targets=True)
            y, taby = limb_cases.element(rs, rnd, my, N_PER_PAIR, weak_targets=True)
            kx, ky = min(len(tabx), half - 1), min(len(taby), half - 1)
            x[1 : 1 + kx] = tabx[:kx]            # every special form of x, one by one ...
            y[1 : 1 + min(kx, ky)] = taby[: min(kx, ky)]  # ... beside a special y
            y[half : half + ky] = taby[:ky]      # every special form of y beside a generated x
            parts.append(np.stack([x, y], axis=1))
    cases = np.concatenate(parts).astype(np.uint32)
    cases.setflags(write=False)
    return cases


def operand_sets():
    """(n, 2, 9) uint32: x limbs, y limbs (read-only, shared)"""
    return _sets()


@functools.lru_cache(maxsize=None)
def reference():
    """(n, 8) uint32 per operand set: the five h160_t words, the parity of y, probe 0's index (low word, high word)"""
    cases = _sets()
    xs, ys = limb_cases.values(cases[:, 0]) % limb_cases.P, limb_cases.values(cases[:, 1]) % limb_cases.P
    raw = limb_cases.values(cases[:, 1])
    # the special forms are there: values that need the final subtraction, and the residues 0, 1, p - 1 of y
    assert {0, 1, limb_cases.P - 1} <= {int(v) for v in ys} and any(int(v) >= limb_cases.P for v in raw)
    out = np.zeros((len(cases), 8), dtype=np.uint32)
    for i in range(len(cases)):
        x, y = int(xs[i]), int(ys[i])
        h = orc.hash160(x, y)
        a0, a1 = h[0] << 32 | h[1], h[2] << 32 | h[3]
        idx = ((a0 << 24) | (a1 >> 24)) & ((1 << 64) - 1)  # bloom.h: probe 0 (S = 24, j = 0)
        out[i] = h + [y & 1, idx & 0xFFFFFFFF, idx >> 32]
    out.setflags(write=False)
    return out
