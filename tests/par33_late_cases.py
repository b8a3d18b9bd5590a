"""Operand sets for the late start of emit33_ypar_short's d stream (csrc/emit33.h: column 8 for its digit, then columns 13..16 with no
carry-in, and a guard on column 14's truncated digit), shared by the CPU test (tests/test_par33_late_host.py) and the GPU test
(tests/test_gpu_par33_late.py, through Device.diag_limbs).

They come from the -late mode of the stand-alone program csrc/tools/par33_host.cpp (tests/par33_cases.py compiles it): seeded random sets
(set 11, the first 1024 kept), limbs 4..8 of both factors at 0 / the ceiling in all 1024 patterns (set 12), sets solved for on both sides
of the new guard (set 13) and sets on which the late start alone gives a wrong u_6 (set 14).  One run per session."""
import functools
import os
import subprocess

import numpy as np

import par33_cases as C

K0 = 4   # EMIT33_YPAR_K0: the d stream starts at column 9 + K0
F = 32   # EMIT33_YPAR_F
M = (1 << 29) - 1


@functools.lru_cache(maxsize=None)
def run(log2_random=22):
    """(exit status, output, records) of one run of par33_host -late"""
    out = os.path.join(C._workdir(), "late_%d.bin" % log2_random)
    pr = subprocess.run([C.program(), "-late", out, str(log2_random)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = pr.stdout.decode(errors="replace")
    recs = np.zeros(0, C.REC)
    if pr.returncode == 0:
        raw = open(out, "rb").read()
        n = int(np.frombuffer(raw[:4], "<u4")[0])
        recs = np.frombuffer(raw[4:], C.REC)
        assert len(recs) == n
    return pr.returncode, text, recs


def d_digits(a, b, k0):
    """digits u_k0..u_7 of fe_mul's d stream in Python integers, started at column 9 + k0 with no carry-in (k0 = None: the whole stream)"""
    a, b = [int(v) for v in a], [int(v) for v in b]
    d = 0 if k0 is not None else sum(a[i] * b[8 - i] for i in range(9)) >> 29
    u = {}
    for k in range(k0 or 0, 8):
        d += sum(a[i] * b[9 + k - i] for i in range(k + 1, 9))
        u[k] = d & M
        d >>= 29
    return u
