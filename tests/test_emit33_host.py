"""csrc/emit33.h on the CPU: the addr33-only emit path of the add kernels (limbs -> SHA-256 message words, y's parity from its top limbs,
probe 0's index from RIPEMD-160's native words) against the composition it replaces and against the oracle.

The stand-alone program csrc/tools/emit33_host.cpp does the comparison with today's fe_normalize + fe_to_words + fe_parity + hash160_33 +
bloom_index, bit for bit: on its built-in cases (20 000 seeded random limb sets, ceilings, multiples of p +- d, values the weak pass
leaves in [p, 2p) with and without bit 24 in limb 8, the top of y swept over the boundary of its parity estimate), and on the operand
sets of tests/limb_cases.py, which this test writes to a file: x at magnitudes 1 .. 4, y at 1 .. 3, every pattern of `element` at
the magnitude ceilings, the weak-pass targets and the table of k p +- d included.  What the program returns for those - hash160, parity,
index - is then compared with the oracle's hash160 of (x mod p, y mod p) and with bloom.h's index formula in Python integers."""
import subprocess

import numpy as np
import pytest

import emit33_cases
from support import host_program


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_program(tmp_path_factory.mktemp("emit33"), "emit33_host.cpp", ["-O2"], sanitize=False)


def test_builtin_cases_agree_with_the_general_path(prog):
    pr = subprocess.run([prog], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = pr.stdout.decode(errors="replace")
    assert pr.returncode == 0 and "cases ok" in out, out[-3000:]
    assert int(out.split()[1]) >= 20000


def test_limb_case_operands_agree_with_the_general_path_and_the_oracle(prog, tmp_path):
    cases = emit33_cases.operand_sets()
    n = len(cases)
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.uint32(n).tobytes() + cases.tobytes())
    pr = subprocess.run([prog, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert pr.returncode == 0, pr.stdout.decode(errors="replace")[-3000:]  # old path == new path on every case
    out = np.fromfile(fout, dtype=np.uint32).reshape(n, 8)
    want = emit33_cases.reference()
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert not len(bad), (int(bad[0]), cases[bad[0]].tolist(), out[bad[0]].tolist(), want[bad[0]].tolist())
