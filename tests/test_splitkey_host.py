"""The split-key vanity search (`-p` with `-k <pubkey>`, `combine`) without a GPU: host/splitkey.h compiled for the host
(csrc/tools/splitkey_host.cpp) against Python integers over the oracle's points; the pins of the C ABI header and the binding; the CLI's
refusals and usage lines, all before a GPU is looked for; `combine` on known triples; the static figures of the two verification kernels."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import orc
from ecloop_amd.capi import limbs
from support import ROOT, cli, host_lib, host_program, int_of, run_program

P, N = orc.P, orc.N
G1 = "0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798"


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    lib = host_lib(tmp_path_factory, "splitkey_host.cpp")
    V = C.c_void_p
    lib.sk_host_image_origin.argtypes = [V, V, C.c_uint]
    lib.sk_host_image_origin.restype = None
    lib.sk_host_endo_scalar.argtypes = [V, C.c_uint, V]
    lib.sk_host_endo_scalar.restype = None
    lib.sk_host_combine.argtypes = [V, V, C.c_uint, V]
    lib.sk_host_combine.restype = None
    return lib


def image_origin(H, pt, e):
    x, y = limbs(pt[0]), limbs(pt[1])
    H.sk_host_image_origin(x.ctypes.data, y.ctypes.data, e)
    return int_of(x), int_of(y)


def combine(H, kq, part, e):
    a, b, out = limbs(kq), limbs(part), np.zeros(4, np.uint64)  # (named: the arrays live until the call returns)
    H.sk_host_combine(a.ctypes.data, b.ctypes.data, e, out.ctypes.data)
    return int_of(out)


def endo_scalar(H, k, e):
    a, out = limbs(k), np.zeros(4, np.uint64)
    H.sk_host_endo_scalar(a.ctypes.data, e, out.ctypes.data)
    return int_of(out)


def image_of(pt, e):
    """image e of a point, from the oracle: the point of the key calc_priv maps a key of pt to - here by the map itself, in integers"""
    from ecloop_amd.engine import SPLITKEY_BETA
    x, y = pt
    return x * pow(SPLITKEY_BETA, e // 2, P) % P, (P - y) % P if e & 1 else y


def test_images_and_combination_for_all_six_images_against_the_oracles_points(H):
    from ecloop_amd.engine import calc_priv, splitkey_combine, splitkey_image_origin
    rng = random.Random("splitkey")
    kqs = [1, 2, 0xDC2A04, N - 1, N - 2] + [rng.randrange(1, N) for _ in range(6)]
    ks = [1, 7, N - 1] + [rng.randrange(1, N) for _ in range(4)]
    for kq in kqs:
        Q = orc.point_of(kq)
        for e in range(6):
            # image e of Q = kq G is the oracle's point of calc_priv(kq, e): the header's, the engine's and the integer form agree
            want = orc.point_of(calc_priv(kq, 1, 0, e))
            assert image_origin(H, Q, e) == want == splitkey_image_origin(Q, e) == image_of(Q, e)
            assert endo_scalar(H, kq, e) == calc_priv(kq, 1, 0, e)
            for k in ks:
                part = calc_priv(k, 1, 0, e)
                fin = combine(H, kq, part, e)
                assert fin == (calc_priv(kq, 1, 0, e) + part) % N == splitkey_combine(kq, part, e)
                if (kq + k) % N == 0:
                    assert fin == 0  # k_Q + k = 0 (mod n): no key (the walk never reports it: Q + k G is the point at infinity)
                    continue
                assert fin != 0 and orc.point_of(fin) == image_of(orc.point_of((kq + k) % N), e)  # the final key's point IS image e of (kQ + k) G
    # the edges by name: k_Q = n - 1 with k = 1 (the sum is 0), k_Q = n - 1 with k = 2 (the sum wraps to 1)
    assert combine(H, N - 1, 1, 0) == 0 and combine(H, N - 1, 2, 0) == 1
    assert combine(H, 5, 7, 0) == 12 and combine(H, 5, N - 7, 1) == (N - 12) % N  # e = 1: -(5) + -(7)
    assert endo_scalar(H, N + 5, 0) == 5 and combine(H, 5, N + 3, 0) == 8  # values of 256 bits are reduced first


def test_header_and_binding_pins():
    from ecloop_amd import capi
    header = open(os.path.join(ROOT, "include", "ecloop_hip.h")).read()
    flags = dict(re.findall(r"#define (ECL_[A-Z0-9]+) (\d+)u", header))
    assert {k: int(v) for k, v in flags.items()} == {"ECL_ADDR33": 1, "ECL_ADDR65": 2, "ECL_ENDO": 4, "ECL_P2SH": 16, "ECL_ETH": 64, "ECL_TR": 128,
                                                    "ECL_PUB": 256, "ECL_ORIGIN": 512, "ECL_INSERT": 1024, "ECL_HERD": 2048, "ECL_PREFIX": 4096}
    assert "exactly the 45 ecl_hip_* functions" in header and len(capi.EXPORTS) == 45 == len(set(capi.EXPORTS))
    assert len(set(re.findall(r"\b(ecl_hip_[a-z0-9_]+)\(", header.split("#ifndef ECLOOP_HIP_H")[1]))) == 45
    assert "each entry of `k` is TWELVE limbs" in header and "ECL_PREFIX | ECL_ORIGIN" in header
    assert (capi.ORIGIN, capi.PREFIX) == (512, 4096)
    lib = os.path.join(ROOT, "ecloop_amd", "libecloop_hip.so")
    if os.path.exists(lib):  # what the built library exports: the 45, nothing else
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.split("\n")
        names = sorted(l.split()[-1] for l in syms if l.strip())
        assert names == sorted(capi.EXPORTS)


class Refused(Exception):
    pass


def test_binding_accepts_the_split_key_device_and_keeps_the_other_refusals(monkeypatch):
    """Device() checks its arguments before the library is asked; a load() that raises shows which combinations got through"""
    from ecloop_amd import capi

    def no_library():
        raise Refused()
    monkeypatch.setattr(capi, "load", no_library)
    for kw in (dict(prefix=True, origin=True), dict(prefix=True, origin=True, endo=True), dict(prefix=True, origin=True, a65=True),
               dict(prefix=True, origin=True, a33=False, a65=True, endo=True), dict(prefix=True, origin=True, a33=False, eth=True),
               dict(prefix=True, origin=True, a33=False, eth=True, endo=True)):
        with pytest.raises(Refused):
            capi.Device(0, **kw)  # accepted: the constructor went on to the library
    for kw in (dict(prefix=True, origin=True, pub=True), dict(prefix=True, origin=True, a33=False, pub=True), dict(prefix=True, origin=True, tr=True),
               dict(prefix=True, origin=True, p2sh=True), dict(prefix=True, origin=True, insert=True), dict(prefix=True, origin=True, herd=True),
               dict(prefix=True, origin=True, a33=False), dict(origin=True), dict(origin=True, endo=True), dict(a33=False, pub=True, origin=True, endo=True),
               dict(a33=False, eth=True, origin=True), dict(prefix=True, insert=True), dict(prefix=True, a33=False, pub=True)):
        with pytest.raises(ValueError):
            capi.Device(0, **kw)
    with pytest.raises(Refused):
        capi.Device(0, a33=False, pub=True, origin=True)  # the giant walk of bsgs, as before


def test_the_host_program_runs_clean_under_the_sanitizers(tmp_path):
    """csrc/tools/splitkey_host.cpp has a main of its own: built as a program with the address and undefined-behaviour sanitizers and run"""
    pr = run_program(host_program(tmp_path, "splitkey_host.cpp", ["-O0"]))
    assert pr.returncode == 0 and "splitkey_host: ok" in pr.stdout, (pr.stdout, pr.stderr)


def refused(cli, args, stdin=None):
    feed = {"input": stdin} if stdin is not None else {"stdin": subprocess.DEVNULL}
    pr = subprocess.run([cli] + args, capture_output=True, text=True, timeout=60, **feed)
    assert pr.returncode == 1 and pr.stdout == "", (pr.stdout, pr.stderr)
    assert "no MI355X GPU visible" not in pr.stderr  # refused before a GPU is looked for
    return pr.stderr


def test_cli_refusals_and_usage_before_a_gpu_is_looked_for(cli, tmp_path):
    for verb in ("add", "rnd"):
        err = refused(cli, [verb, "-k", G1, "-r", "1000:2000"])  # (until now -k was silently ignored here)
        assert "-k goes with -p" in err
        assert "-k goes with -p" in refused(cli, [verb, "-k", G1, "-a", "e", "-r", "1000:2000"])
        err = refused(cli, [verb, "-k", G1, "-f", "x.blf", "-r", "1000:2000"])
        assert "-k and -f exclude each other" in err and "-p" in err
    assert "-k and -f exclude each other" in refused(cli, ["add", "-p", "1Love", "-k", G1, "-f", "x.blf", "-r", "1000:2000"])
    assert "-k is not supported with mul" in refused(cli, ["mul", "-k", G1])
    assert "-k is not supported with mul" in refused(cli, ["mul", "-p", "1Love", "-k", G1])
    # exactly one key: a bare x names two, a key off the curve, a file of several
    x = G1[2:]
    assert "a bare x names two keys" in refused(cli, ["add", "-p", "1Love", "-k", x, "-r", "1000:2000"])
    assert "invalid public key" in refused(cli, ["add", "-p", "1Love", "-k", "04" + x + "%064x" % 5, "-r", "1000:2000"])
    assert "invalid public key" in refused(cli, ["add", "-p", "1Love", "-k", "05" + x, "-r", "1000:2000"])
    f = tmp_path / "keys.txt"
    f.write_text(G1 + "\n03" + x + "\n")
    assert "takes one public key" in refused(cli, ["add", "-p", "1Love", "-k", str(f), "-r", "1000:2000"])
    # the pattern is still planned first: its refusals are -p's
    assert "a 0x pattern needs -a e" in refused(cli, ["add", "-p", "0xdeadbeef", "-k", G1, "-r", "1000:2000"])
    assert "-p is not supported with -a s" in refused(cli, ["add", "-p", "1Love", "-k", G1, "-a", "s", "-r", "1000:2000"])
    # -t above 1 is not refused: with a good key and pattern the run gets as far as looking for a GPU (or, with one, runs)
    pr = subprocess.run([cli, "add", "-p", "1Love", "-k", G1, "-t", "2", "-r", "1000:2000"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0 or "no MI355X GPU visible" in pr.stderr, pr.stderr
    for args in ([], ["-h"]):
        out = subprocess.run([cli] + args, capture_output=True, text=True, timeout=60).stdout
        assert "-k <pubkey>     - add, rnd with -p: split-key search" in out and "PARTIAL keys" in out and "split:<e>" in out
        assert "combine         - combine -part <partial key> [-split <e>]" in out and "never type it on the searcher's machine" in out
    # combine's own refusals
    assert "combine -part <partial key>" in refused(cli, ["combine"], stdin="5\n")
    assert "combine -part <partial key>" in refused(cli, ["combine", "-part", "xyz"], stdin="5\n")
    assert "combine -part <partial key>" in refused(cli, ["combine", "-part", "%x" % N], stdin="5\n")
    assert "invalid -split '6'" in refused(cli, ["combine", "-part", "7", "-split", "6"], stdin="5\n")
    for bad in ("", "\n", "0\n", "%x\n" % N, "12g4\n", "1" * 65 + "\n"):
        assert "reads the owner's private key from stdin" in refused(cli, ["combine", "-part", "7"], stdin=bad)
    assert "the combined key is 0" in refused(cli, ["combine", "-part", "1"], stdin="%x\n" % (N - 1))


def test_cli_combine_on_known_triples(cli):
    from ecloop_amd.engine import calc_priv
    rng = random.Random("combine")
    triples = [(5, 7, 0, 12), (5, 7, 1, (N - 5 + 7) % N), (N - 1, 2, 0, 1), (0xDC2A04, 0x1234, 0, 0xDC3C38)]
    for _ in range(12):
        kq, part, e = rng.randrange(1, N), rng.randrange(1, N), rng.randrange(6)
        triples.append((kq, part, e, (calc_priv(kq, 1, 0, e) + part) % N))
    for kq, part, e, want in triples:
        args = ["combine", "-part", "%064x" % part] + (["-split", str(e)] if e else [])
        pr = subprocess.run([cli] + args, input="  0x%X  \n" % kq if e & 1 else "%x\n" % kq, capture_output=True, text=True, timeout=120)
        assert pr.returncode == 0, pr.stderr
        assert pr.stdout.splitlines()[0] == "key: %064x" % want
        assert "%064x" % kq not in pr.stdout + pr.stderr  # the owner's key is never echoed


def test_the_new_kernels_registers_and_loops():
    """tools/isa_mix.py --splitkey on the assembly of the shipped code object: the two verification kernels run under __launch_bounds__(64) with
    no spill and no scratch instruction in the window loop, which is k_verify's own; what they add to k_verify / k_verify_eth is the one
    complete mixed addition (the figures DESIGN section 7 (f12) states)"""
    import sys
    from ecloop_amd.build import build_library
    build_library()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_mix
    r = isa_mix.analyse_splitkey()
    assert set(r) == {"verify origin", "verify origin eth"}
    asm = open(isa_mix.ASM).read()
    for label, v in r.items():
        k, m = v["kernel"], v["mirror"]
        assert k["registers"]["vgpr_spill_count"] == 0 and k["registers"]["sgpr_spill_count"] == 0 and k["registers"]["group_segment_fixed_size"] == 0
        assert k["registers"]["vgpr_count"] <= 128 and k["registers"]["vgpr_count"] == m["registers"]["vgpr_count"]
        assert k["registers"]["private_segment_fixed_size"] == m["registers"]["private_segment_fixed_size"]  # the inversion's, out of line, as in k_verify
        assert k["window_loop_scratch"] == 0 and k["total"]["scratch"] == 0 and len(k["loops"]) == 1
        assert abs(k["window_loop"]["valu"] - m["window_loop"]["valu"]) <= 8 and k["window_loop"]["mad64"] == m["window_loop"]["mad64"]
        extra = k["total"]["valu"] - m["total"]["valu"]
        assert 3000 < extra < 4000, extra  # one jac_madd with its doubling branch, inlined: the window loop's body again
        assert re.search(r"\.amdhsa_kernel %s\b" % re.escape(k["name"]), asm)
        blk = asm[asm.index(".amdhsa_kernel " + k["name"]):]
        assert re.search(r"\.amdhsa_next_free_vgpr \d+", blk)
    # DESIGN's figures, to the 1 % tests/test_profiles_fresh.py allows a fresh build
    assert r["verify origin"]["kernel"]["registers"]["vgpr_count"] == 120 and abs(r["verify origin"]["kernel"]["total"]["valu"] - 13467) <= 134
    assert abs(r["verify origin eth"]["kernel"]["total"]["valu"] - 11940) <= 119
