"""Taproot (-a t, ECL_TR) without a GPU: the yardstick (tests/tr_ref.py) pinned to the BIP341 wallet vector and three private-key known
answers; tools/p2tr_keys.py on their addresses and on what it must refuse; the Taproot pieces of the device headers compiled for the host
(csrc/tools/tr_host.cpp) against the yardstick; the C ABI header and the Python binding; the CLI's help text, refusals and strict list
reader; and, from the assembly the build keeps, the registers and loops of the new kernels."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import orc
import tr_ref
from support import ROOT, cli, host_lib, int_of_words, kept_assembly, words8

sys.path.insert(0, os.path.join(ROOT, "tools"))

TAG = "e80fe1639c9ca050e3af1b39c143c63e429cbceb15d940fbb5c5a1f4af57c5e9"
# BIP341 wallet vector 1 (no script tree): internal key, tweak, output key, address
V1_X = 0xd6889cb081036e0faefa3a35157ad71086b123b2b144b649798b494c300a961d
V1_T = 0xb86e7be8f39bab32a6f2c0443abbc210f0edac0e2c53d501b36b64437d9c6c70
V1_Q = 0x53a1f6e454df1aa2776a2814a721372d6258050de330b3c6d10ee8f4e0dda343
V1_ADDR = "bc1p2wsldez5mud2yam29q22wgfh9439spgduvct83k3pm50fcxa5dps59h4z5"
# private key -> output key
KNOWN = {1: 0xda4710964f7852695de2da025290e24af6d8c281de5a0b902b7135fd9fd74d21,
         2: 0xcafd90c7026f0b6ab98df89490d02732881f2f4b5900856358dddff4679c2ffb,
         0xdc2a04: 0x509eeff5f103f2767a17d3289d857dd538a62a9449646107e5b4b6d0a7898714}
K1_ADDR = "bc1pmfr3p9j00pfxjh0zmgp99y8zftmd3s5pmedqhyptwy6lm87hf5sspknck9"


def y_of(x):
    y = pow(x ** 3 + 7, (orc.P + 1) // 4, orc.P)
    assert y * y % orc.P == (x ** 3 + 7) % orc.P
    return y


def test_the_yardstick_gives_the_published_vector_and_the_known_answers():
    assert tr_ref.TAG.hex() == TAG
    assert tr_ref.tweak(V1_X) == V1_T
    for y in (y_of(V1_X), orc.P - y_of(V1_X)):  # either point with that x: the lift decides
        assert tr_ref.output_key_of_point(V1_X, y) == V1_Q
    assert tr_ref.p2tr_address(V1_Q) == V1_ADDR
    for k, q in KNOWN.items():
        assert tr_ref.output_key(k) == q, hex(k)
        assert tr_ref.output_key(orc.N - k) == q  # k and n - k share the output key
    assert tr_ref.p2tr_address(KNOWN[1]) == K1_ADDR
    assert tr_ref.output_key(0) is None and tr_ref.output_key(orc.N) is None
    assert tr_ref.mul_g(12345) == orc.point_of(12345)  # the yardstick's own arithmetic against the oracle's points


def p2tr_keys(text):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "p2tr_keys.py")], input=text, capture_output=True, text=True, timeout=60)


def test_p2tr_keys_decodes_the_addresses_and_refuses_everything_else():
    pr = p2tr_keys(V1_ADDR + "\n\n" + K1_ADDR.upper() + "\n")
    assert pr.returncode == 0 and pr.stdout.split() == ["%064x" % V1_Q, "%064x" % KNOWN[1]], (pr.stdout, pr.stderr)
    flipped = V1_ADDR[:20] + ("q" if V1_ADDR[20] != "q" else "p") + V1_ADDR[21:]
    v0 = "bc1qw508d6qejxtdg4y5r3zarvary0c5xw7kv8f3t4"  # BIP173's P2WPKH example: witness version 0, bech32
    # a version-1 program under a bech32 (not -m) checksum: the address re-encoded with the other constant
    data = [tr_ref.CHARSET.index(c) for c in V1_ADDR[3:-6]]
    pm = tr_ref._polymod([3, 3, 0, 2, 3] + data + [0] * 6) ^ 1
    bech32 = "bc1" + V1_ADDR[3:-6] + "".join(tr_ref.CHARSET[pm >> 5 * (5 - i) & 31] for i in range(6))
    for bad in (v0, bech32, flipped, V1_ADDR[:-1], "bc1p", "hello"):
        pr = p2tr_keys(K1_ADDR + "\n" + bad + "\n")
        assert pr.returncode != 0 and pr.stdout.split() == ["%064x" % KNOWN[1]] and bad in pr.stderr, (bad, pr.stdout, pr.stderr)


@pytest.fixture(scope="module")
def T(tmp_path_factory):
    lib = host_lib(tmp_path_factory, "tr_host.cpp")
    lib.th_tweak_many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.th_ge_n_many.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.th_lift_many.argtypes = [C.c_void_p, C.c_uint32]
    lib.th_add_x.argtypes = [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 3
    lib.th_add_x.restype = C.c_int
    return lib


def test_taptweak_of_the_device_header_equals_the_yardstick(T):
    rnd = random.Random(341)
    xs = [V1_X, 0, (1 << 256) - 1] + [rnd.getrandbits(256) for _ in range(10000)]  # any words: they need not be x coordinates
    X = np.array([words8(x) for x in xs], np.uint32)
    tw = np.zeros_like(X)
    ge = np.zeros(len(X), np.uint8)
    T.th_tweak_many(X.ctypes.data, tw.ctypes.data, ge.ctypes.data, len(X))
    assert int_of_words(tw[0]) == V1_T
    for i, x in enumerate(xs):
        t = tr_ref.tweak(x)
        assert int_of_words(tw[i]) == t and bool(ge[i]) == (t >= orc.N), i


def test_the_tweak_range_test_and_the_even_y_lift(T):
    ts = [orc.N - 1, orc.N, orc.N + 1, (1 << 256) - 1, 0, 1, orc.N - (1 << 32), orc.N + (1 << 64), 1 << 255]
    W = np.array([words8(t) for t in ts], np.uint32)
    ge = np.zeros(len(W), np.uint8)
    T.th_ge_n_many(W.ctypes.data, ge.ctypes.data, len(W))
    assert [bool(g) for g in ge] == [t >= orc.N for t in ts]
    ys = [orc.point_of(k)[1] for k in range(1, 40)] + [1, 2, orc.P - 1, orc.P - 2]
    assert {y & 1 for y in ys} == {0, 1}  # both parities
    Y = np.array([words8(y) for y in ys], np.uint32)
    T.th_lift_many(Y.ctypes.data, len(Y))
    for i, y in enumerate(ys):
        assert int_of_words(Y[i]) == (y if y % 2 == 0 else orc.P - y), i


def add_x(T, t, p):
    tx, ty = (0, 0) if t is None else t
    a = [np.array(words8(v), np.uint32) for v in (tx, ty, p[0], p[1])]
    out = np.zeros(8, np.uint32)
    how = T.th_add_x(a[0].ctypes.data, a[1].ctypes.data, int(t is None), a[2].ctypes.data, a[3].ctypes.data, out.ctypes.data)
    return how, int_of_words(out)


def test_the_addition_of_stage_b_and_its_exceptional_cases(T):
    """the XYZZ + affine addition k_tr_check closes a key with, and the complete formulas it falls back to where that leaves ZZ = 0:
    T = P' (the tangent), T = -P' (no output key), T = infinity (t = 0: Q = P'), against Python"""
    rnd = random.Random(86)
    for _ in range(200):
        a, b = rnd.randrange(1, orc.N), rnd.randrange(1, orc.N)
        if a in (b, orc.N - b):
            continue
        pa, pb = orc.point_of(a), orc.point_of(b)
        assert add_x(T, pa, pb) == (1, tr_ref.add(pa, pb)[0])  # the ordinary case stays on the lazy path
    for k in (1, 2, 7, 0xdc2a04, orc.N - 5):
        p = orc.point_of(k)
        neg = (p[0], orc.P - p[1])
        assert add_x(T, p, p) == (2, tr_ref.add(p, p)[0]), k      # T = P'
        assert add_x(T, neg, p)[0] == 0, k                        # T = -P'
        assert add_x(T, None, p) == (2, p[0]), k                  # T = infinity


def test_header_and_binding_declare_taproot():
    header = open(os.path.join(ROOT, "include", "ecloop_hip.h")).read()
    assert re.search(r"#define ECL_TR 128u\b", header)
    assert re.search(r"int ecl_hip_verify_tr\(ecl_hip \*h, const uint64_t \(\*k\)\[4\], uint32_t n, uint32_t \(\*qx\)\[8\], uint8_t \*ok\);", header)
    assert re.search(r"int ecl_hip_diag_tr\(ecl_hip \*h, const uint64_t \(\*x\)\[4\], const uint64_t \(\*y\)\[4\], uint64_t \(\*t\)\[4\], uint32_t \(\*qx\)\[8\], "
                     r"uint8_t \*ok, uint32_t n\);", header)
    assert "taproot is searched alone" in header.lower()
    assert "exactly the 45 ecl_hip_* functions" in header
    from ecloop_amd import capi
    assert capi.TR == 128 and capi.label_of(4) == "p2tr" and len(capi.EXPORTS) == 45
    assert "ecl_hip_verify_tr" in capi.EXPORTS and "ecl_hip_diag_tr" in capi.EXPORTS
    exports = open(os.path.join(ROOT, "ecloop_amd", "csrc", "exports.map")).read()
    assert "ecl_hip_*" in exports


def test_cli_help_names_the_letter_and_mixed_type_strings_are_refused(cli):
    out = subprocess.run([cli], capture_output=True, text=True, timeout=60).stdout
    line = [l for l in out.splitlines() if l.strip().startswith("-a ")]
    assert len(line) == 1 and re.search(r"\bt - p2tr \(Taproot, bc1p\.\.\.\)", line[0]), out
    for verb in ("add", "mul", "rnd"):
        for extra in (["-a", "ct"], ["-a", "te"], ["-a", "ts"], ["-a", "ut"], ["-a", "t", "-endo"]):  # before the filter is opened or a GPU looked for
            pr = subprocess.run([cli, verb] + extra + ["-f", "/nonexistent", "-r", "8000:ffff"], stdin=subprocess.DEVNULL, capture_output=True,
                                text=True, timeout=60)
            assert pr.returncode != 0 and "taproot is searched alone" in pr.stderr and "nonexistent" not in pr.stderr, (verb, extra, pr.stderr)


@pytest.mark.parametrize("decoder", ["ssse3", "scalar"])
def test_blf_gen_reads_64_digit_lines_strictly_with_a_t_only(cli, tmp_path, decoder):
    """blf-gen (host path: a small filter) then blf-check over a file that mixes 64-digit, 40-digit and 0x-prefixed lines: with -a t exactly
    the 64-digit lines are entries (their leading 40 digits); without it the file gives what it always gave - one entry per 64-digit and
    per 40-digit line (the rule that every full 40-character piece of a line is an entry)"""
    env = dict(os.environ, **({"ECLOOP_HIP_NO_SSSE3": "1"} if decoder == "scalar" else {}))
    keys = ["%064x" % q for q in list(KNOWN.values()) + [V1_Q]]
    forty = ["751e76e8199196d454941c45d1b3a323f1433bd6", "7025b4efb3ff42eb4d6d71fab6b53b4f4967e3dd"]
    junk = ["0x" + keys[0], "0x" + forty[0], keys[1][:63], keys[2] + "0", keys[3][:40] + "zz" + keys[3][42:], "g" * 64]
    text = "\n".join([keys[0], forty[0], junk[0], keys[1].upper(), junk[1], junk[2], keys[2], forty[1], junk[3], junk[4], junk[5], keys[3]]) + "\n"
    ask = [k[:40] for k in keys] + forty
    # what the lines give under the default rule: keys[2] + "0" is 65 characters (one piece), 0x + 64 digits is 66 (one piece, not hex),
    # 0x + 40 digits is 42 (one piece, not hex), 63 digits is one piece (the first 40 of keys[1], which the upper-case line gives too),
    # the line with zz has a clean first piece; "g" * 64 none
    default = {k[:40] for k in keys} | set(forty)
    for with_t, want in ((True, {k[:40] for k in keys}), (False, default)):
        blf = str(tmp_path / ("l%d.blf" % with_t))
        pr = subprocess.run([cli, "blf-gen", "-n", "1000", "-o", blf] + (["-a", "t"] if with_t else []), input=text.encode(), capture_output=True,
                            timeout=120, env=env)
        assert pr.returncode == 0, pr.stderr
        assert b"added %d new items" % len(want) in pr.stdout, (with_t, pr.stdout)
        pr = subprocess.run([cli, "blf-check", "-f", blf] + ask, capture_output=True, text=True, timeout=120, env=env)
        found = {l.split()[0] for l in pr.stdout.splitlines() if l.endswith(" FOUND") and not l.endswith("NOT FOUND")}
        assert found == want, (with_t, pr.stdout)
    # a hash160 list given to a Taproot search by mistake holds no entry
    lst = tmp_path / "p2pkh.txt"
    lst.write_text("\n".join(forty) + "\n")
    pr = subprocess.run([cli, "add", "-a", "t", "-f", str(lst), "-r", "8000:ffff"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60)
    assert pr.returncode != 0 and "no hashes in filter file" in pr.stderr


def test_the_new_kernels_fit_168_registers_and_keep_scratch_out_of_their_loops():
    """static, from the assembly the build keeps (tools/isa_mix.py: analyse_tr): each Taproot kernel has at most 168 VGPRs and no scratch
    instruction in any loop below its launch loop (k_add_tr) / its round loops (the others) - and none in the round loops either, the
    arguments of the out-of-line complete sum aside; the window loop holds the 918 multiply-adds of one XYZZ addition"""
    import isa_mix
    now = isa_mix.analyse_tr(kept_assembly())
    assert set(now) == set(isa_mix.TR_KERNELS) and len(now) == 4
    for label, a in now.items():
        print(label, a["registers"], {k: v for k, v in a.items() if k.startswith(("scratch", "window", "walk", "tagged"))})
        assert a["registers"]["vgpr_count"] <= 168, (label, a["registers"])
        assert a["loops"] and a["scratch_below_top"] == 0, (label, a["loops"])
        if label != "-a t emit":
            assert a["scratch_in_round_loops"] == 0 and a["window_loop_mad64"] == 918, (label, a)
    assert any(l["depth"] >= 3 for l in now["-a t emit"]["loops"])  # launch > table > `which`: the loop nest was seen
    assert 1500 < now["-a t emit"]["tagged_hash_loop_valu"] < 2600  # curve arithmetic + normalisation + one SHA-256 compression, no hash160
