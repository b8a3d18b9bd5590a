"""P2SH-P2WPKH (-a s) without a GPU: hash160_p2sh of the device header hash160.h compiled for the host and checked against known
answers and against hashlib SHA-256 + the oracle's RIPEMD-160; the C ABI header's flag and entry point; the CLI's help text."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import orc
import p2sh_ref
from support import ROOT, host_lib

# private key -> (hash160 of the compressed key, its P2SH-P2WPKH hash); key 1 is the address 3JvL6Ymt8MVWiCNHC7oWU6nLeHNJKLZGLN
KNOWN = {1: ("751e76e8199196d454941c45d1b3a323f1433bd6", "bcfeb728b584253d5f3f70bcb780e9ef218a68f4"),
         2: ("06afd46bcdfd22ef94ac122aa11f241244a37ecc", "978a0121f9a24de65a13bab0c43c3a48be074eae"),
         0xdc2a04: ("0959e80121f36aea13b3bad361c15dac26189e2f", "45a41e75045f683ed5f71fec4b4322fcd263891b")}


@pytest.fixture(scope="module")
def P(tmp_path_factory):
    lib = host_lib(tmp_path_factory, "p2sh_host.cpp")
    lib.ph_p2sh_many.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    return lib


def device_p2sh(P, h33):
    H = np.ascontiguousarray(h33, dtype=np.uint32).reshape(-1, 5)
    out = np.zeros_like(H)
    P.ph_p2sh_many(H.ctypes.data, out.ctypes.data, len(H))
    return out


def test_known_answers(P):
    for k, (h33, want) in KNOWN.items():
        x, y = orc.point_of(k)
        assert orc.hex160(orc.hash160(x, y, True)) == h33  # the table's first column, from the oracle
        got = device_p2sh(P, [int(h33[i:i + 8], 16) for i in range(0, 40, 8)])[0]
        assert orc.hex160(got) == want, k
        assert p2sh_ref.p2sh_hex(h33) == want  # ... and the reference computation the other tests use


def test_random_hashes_against_hashlib_and_the_oracle_ripemd(P):
    rng = np.random.default_rng(49)
    H = rng.integers(0, 1 << 32, size=(10240, 5), dtype=np.uint64).astype(np.uint32)
    H[0], H[1] = 0, 0xFFFFFFFF  # all-zero and all-ones inputs
    got = device_p2sh(P, H)
    for i in range(len(H)):
        assert [int(v) for v in got[i]] == p2sh_ref.p2sh_of_h33(H[i]), i


def test_header_declares_the_flag_and_the_entry_point():
    header = open(os.path.join(ROOT, "include", "ecloop_hip.h")).read()
    assert re.search(r"#define ECL_P2SH 16u\b", header)  # (8 stays an unknown flag: tests/test_gpu_primitives.py)
    assert re.search(r"int ecl_hip_p2sh_hash\(ecl_hip \*h, const uint32_t \(\*h33\)\[5\], uint32_t \(\*out\)\[5\], uint32_t n\);", header)
    from ecloop_amd import capi
    assert capi.P2SH == 16 and "ecl_hip_p2sh_hash" in capi.EXPORTS and capi.label_of(2) == "p2sh"


def test_cli_help_names_the_p2sh_letter():
    from ecloop_amd.build import build_host_cli, build_library
    build_library()
    exe = build_host_cli()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout
    line = [l for l in out.splitlines() if l.strip().startswith("-a ")]
    assert len(line) == 1 and re.search(r"\bs - p2sh\b", line[0]), out
