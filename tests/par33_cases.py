"""Operand sets for emit33_ypar (csrc/emit33.h: the parity of y = lam b - Y of a walked point from a partial product), shared by the CPU
test (tests/test_par33_host.py) and the GPU test (tests/test_gpu_par33.py, through Device.diag_limbs).

The stand-alone program csrc/tools/par33_host.cpp makes them and checks each against fe_parity(fe_sub(fe_mul(lam, b), Y)) and against
big-number arithmetic of its own: seeded random sets (set 1), limbs 5..8 of both factors at 0 / the ceiling in every pattern (set 2), sets
on both sides of the guard found by its search (set 3), and sets on which the short way alone is wrong (set 4).  It is compiled and run
once per session; the records it writes - operands, parity, path taken - are what the device has to reproduce."""
import functools
import os
import subprocess
import tempfile

import numpy as np

from support import host_program

LIMB_PAR33 = 27  # csrc/limb_ops.h: in0 = lam, in1 = b, in2 = Y; flag = parity, out0.n[0] = 1 when the exact product was taken
G = 256          # EMIT33_YPAR_G
REC = np.dtype([("lam", "<u4", 9), ("b", "<u4", 9), ("Y", "<u4", 9), ("par", "<u4"), ("path", "<u4"), ("set", "<u4")])
P = (1 << 256) - (1 << 32) - 977

_dir = None


def _workdir():
    global _dir
    if _dir is None:
        _dir = tempfile.TemporaryDirectory(prefix="par33")
    return _dir.name


@functools.lru_cache(maxsize=None)
def program(sanitize=False):
    """path of the compiled program (g++; with sanitize: the address and undefined-behaviour sanitizers, errors fatal)"""
    return host_program(_workdir(), "par33_host.cpp", ["-O1", "-g"] if sanitize else ["-O2"], sanitize)


@functools.lru_cache(maxsize=None)
def run(log2_random=22, sanitize=False):
    """(exit status, output, records) of one run; the records are sets 2..4 whole and the first 4096 of set 1"""
    out = os.path.join(_workdir(), "cases_%d_%d.bin" % (log2_random, sanitize))
    pr = subprocess.run([program(sanitize), out, str(log2_random)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = pr.stdout.decode(errors="replace")
    recs = np.zeros(0, REC)
    if pr.returncode == 0:
        raw = open(out, "rb").read()
        n = int(np.frombuffer(raw[:4], "<u4")[0])
        recs = np.frombuffer(raw[4:], REC)
        assert len(recs) == n
    return pr.returncode, text, recs


def values(limbs):
    """Python integers of (n, 9) raw limbs"""
    return [sum(int(v) << (29 * i) for i, v in enumerate(row)) for row in limbs]
