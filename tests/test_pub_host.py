"""Public keys by x (-a x, ECL_PUB) without a GPU: the device header's x-only arithmetic (csrc/pub_emit.h) compiled for the host
(csrc/tools/pub_host.cpp) against Python arithmetic on the oracle's points; the yardstick (tests/pub_ref.py) against the oracle; the C ABI
header and the Python binding; the CLI's help text, refusals and strict list reader; and, from the assembly the build keeps, the registers,
loops and static per-key instruction count of the new kernels."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import orc
import pub_ref
from support import ROOT, cli, host_lib, int_of_words, kept_assembly, words8

sys.path.insert(0, os.path.join(ROOT, "tools"))
P, N = orc.P, orc.N


def y_of(x):
    """a y with y^2 = x^3 + 7, or None"""
    y = pow(x ** 3 + 7, (P + 1) // 4, P)
    return y if y * y % P == (x ** 3 + 7) % P else None


def pair_x(c, g):
    """x of C + G and of C - G by the affine formulas, in Python"""
    inv = pow((g[0] - c[0]) % P, P - 2, P)
    lp, lm = (g[1] - c[1]) * inv % P, (-g[1] - c[1]) * inv % P
    return (lp * lp - c[0] - g[0]) % P, (lm * lm - c[0] - g[0]) % P


def test_the_yardstick_against_the_oracle():
    """x(lambda k) = beta x(k), x(-k) = x(k): the three images the yardstick gives are the x of calc_priv's six keys"""
    assert pow(pub_ref.BETA, 3, P) == 1 and pow(pub_ref.LAMBDA, 3, N) == 1
    for k in (1, 2, 0xdc2a04, N - 5, 0x123456789abcdef):
        im = pub_ref.endo_images(k)
        for endo in range(6):
            assert tuple(pub_ref.words5(orc.point_of(pub_ref.calc_priv(k, endo))[0])) == im[endo & ~1], (k, endo)
        assert pub_ref.h160_of(k) == im[0] == pub_ref.h160_of(N - k)
        x, y = orc.point_of(k)
        assert pub_ref.compressed(k) == ("03" if y & 1 else "02") + "%064x" % x
        assert pub_ref.compressed(N - k)[2:] == pub_ref.compressed(k)[2:] and pub_ref.compressed(N - k)[:2] != pub_ref.compressed(k)[:2]
    assert pub_ref.compressed(1) == "0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798"
    assert pub_ref.x_of(0) is None and pub_ref.x_of(N) is None


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    lib = host_lib(tmp_path_factory, "pub_host.cpp")
    lib.ph_pair_many.argtypes = [C.c_void_p] * 6 + [C.c_uint32]
    lib.ph_probe_many.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    return lib


def pairs_on_device_header(H, cs, gs):
    arr = [np.array([words8(v) for v in col], np.uint32) for col in ([c[0] for c in cs], [c[1] for c in cs], [g[0] for g in gs], [g[1] for g in gs])]
    xp, xm = np.zeros_like(arr[0]), np.zeros_like(arr[0])
    H.ph_pair_many(*[a.ctypes.data for a in arr], xp.ctypes.data, xm.ctypes.data, len(cs))
    return [int_of_words(w) for w in xp], [int_of_words(w) for w in xm]


def test_the_x_only_pair_step_of_the_device_header(H):
    """10 000 random pairs (centre, table point) of the oracle's points: x of C + G and C - G from pub_pair_x equal Python's; then the edge
    cases - Gx - X of either sign and tiny, a centre whose x is just below p, x values with leading zero bytes"""
    rnd = random.Random(256)
    cs, gs = [], []
    base = [orc.point_of(rnd.randrange(1, N)) for _ in range(200)]
    tab = [orc.point_of(i + 1) for i in range(50)]
    for _ in range(10000):
        c, g = rnd.choice(base), rnd.choice(tab)
        if c[0] == g[0]:
            continue
        cs.append(c), gs.append(g)
    # either sign of Gx - X: every (c, g) also as (g, c)
    n0 = len(cs)
    cs, gs = cs + gs[:500], gs + cs[:500]
    signs = {(g[0] > c[0]) for c, g in zip(cs, gs)}
    assert signs == {True, False}
    xp, xm = pairs_on_device_header(H, cs, gs)
    for i, (c, g) in enumerate(zip(cs, gs)):
        assert (xp[i], xm[i]) == pair_x(c, g), i
    # the sums are the oracle's points: C + G = (kc + kg) G
    kc, kg = 0x1234567, 33
    xp, xm = pairs_on_device_header(H, [orc.point_of(kc)], [orc.point_of(kg)])
    assert xp[0] == orc.point_of(kc + kg)[0] and xm[0] == orc.point_of(kc - kg)[0]
    assert n0 > 9000


def near_p_points(count):
    """curve points whose x is just below p (the arithmetic never sees them from a scalar: built from x)"""
    out, x = [], P - 1
    while len(out) < count:
        y = y_of(x)
        if y is not None:
            out.append((x, y))
        x -= 1
    return out


def small_x_points(count):
    """curve points whose x has leading zero bytes (x < 2^200, 2^96, 2^32 ...)"""
    out = []
    for bits in (200, 160, 96, 64, 32, 8):
        x = (1 << bits) - 1
        got = 0
        while got < count:
            y = y_of(x)
            if y is not None:
                out.append((x, y))
                got += 1
            x -= 1
    return out


def test_edge_cases_of_the_pair_step_and_the_probed_words(H):
    edge = near_p_points(6) + small_x_points(2)
    tab = [orc.point_of(i + 1) for i in range(4)]
    cs, gs = [], []
    for c in edge:
        for g in tab + edge:
            if c[0] != g[0]:
                cs.append(c), gs.append(g)  # (an edge point as the table side too: Gx - X tiny, of either sign)
    xp, xm = pairs_on_device_header(H, cs, gs)
    for i, (c, g) in enumerate(zip(cs, gs)):
        assert (xp[i], xm[i]) == pair_x(c, g), (i, hex(c[0]), hex(g[0]))
    # the probed words: x just below p, x with leading zero bytes, 0 and 1, and random x - at every magnitude a walked x arrives in
    rnd = random.Random(20)
    xs = [P - 1, P - 2, P - 0x3D1, 1, 0, 2 ** 32 + 976, 1 << 255, (1 << 96) - 1, 0xFF, (1 << 224) + 5] + [c[0] for c in edge] + \
         [rnd.randrange(P) for _ in range(2000)]
    X = np.array([words8(x) for x in xs], np.uint32)
    for mag in (1, 2, 4):
        h = np.zeros((len(xs), 15), np.uint32)
        H.ph_probe_many(X.ctypes.data, mag, h.ctypes.data, len(xs))
        for i, x in enumerate(xs):
            want = pub_ref.words5(x) + pub_ref.words5(pub_ref.BETA * x % P) + pub_ref.words5(pub_ref.BETA * pub_ref.BETA * x % P)
            assert [int(v) for v in h[i]] == want, (mag, hex(x))
    assert pub_ref.words5(0xFF) == [0, 0, 0, 0, 0] and pub_ref.words5(P - 1)[0] == 0xFFFFFFFF


def test_header_and_binding_declare_pub():
    header = open(os.path.join(ROOT, "include", "ecloop_hip.h")).read()
    assert re.search(r"#define ECL_PUB 256u\b", header)
    assert "public keys are searched alone" in header.lower()
    assert "exactly the 45 ecl_hip_* functions" in header
    from ecloop_amd import capi
    assert capi.PUB == 256 and capi.label_of(5) == "pub" and len(capi.EXPORTS) == 45
    src = open(os.path.join(ROOT, "ecloop_amd", "capi.py")).read()
    assert "def verify_pub(" in src
    with pytest.raises(ValueError):
        capi.Device(0, pub=True)  # a33 defaults to True: refused before the library is asked (no GPU is needed to get here)
    for kw in ({"a65": True}, {"p2sh": True}, {"eth": True}, {"tr": True}):
        with pytest.raises(ValueError):
            capi.Device(0, a33=False, pub=True, **kw)


def test_cli_help_names_the_letter_and_mixed_type_strings_are_refused(cli):
    out = subprocess.run([cli], capture_output=True, text=True, timeout=60).stdout
    line = [l for l in out.splitlines() if l.strip().startswith("-a ")]
    assert len(line) == 1 and "x - pubkey (public key, by its x coordinate)" in line[0], out
    for verb in ("add", "mul", "rnd", "blf-gen"):
        for addr in ("cx", "xc", "ux", "xs", "xe", "xt", "cux"):  # before the filter is opened or a GPU looked for
            for endo in ([], ["-endo"]):
                pr = subprocess.run([cli, verb, "-a", addr] + endo + ["-f", "/nonexistent", "-r", "8000:ffff"], stdin=subprocess.DEVNULL,
                                    capture_output=True, text=True, timeout=60)
                assert pr.returncode != 0 and "public keys are searched alone" in pr.stderr and "nonexistent" not in pr.stderr, (verb, addr, pr.stderr)
    # -a x alone, with or without -endo, gets as far as the filter
    for endo in ([], ["-endo"]):
        pr = subprocess.run([cli, "add", "-a", "x"] + endo + ["-f", "/nonexistent", "-r", "8000:ffff"], stdin=subprocess.DEVNULL, capture_output=True,
                            text=True, timeout=60)
        assert pr.returncode != 0 and "failed to open filter file" in pr.stderr, pr.stderr


@pytest.mark.parametrize("decoder", ["ssse3", "scalar"])
def test_blf_gen_reads_public_keys_strictly_with_a_x_only(cli, tmp_path, decoder):
    """blf-gen (host path: a small filter) then blf-check over a file that mixes 64-, 66- and 130-digit lines, 05-prefixed lines, off-curve
    04 lines, 40-digit lines and 0x-prefixed lines: with -a x exactly the public keys are entries (the leading 40 digits of their x);
    without it the file gives what it always gave - one entry per full clean 40-character piece of a line"""
    env = dict(os.environ, **({"ECLOOP_HIP_NO_SSSE3": "1"} if decoder == "scalar" else {}))
    pts = [orc.point_of(k) for k in (1, 2, 0xdc2a04, 7, 8, 9, 10, 11, 12, 13)]
    hx = lambda v: "%064x" % v
    bare = [hx(pts[0][0]), hx(pts[1][0]).upper()]
    comp = ["%02x" % (2 | (pts[2][1] & 1)) + hx(pts[2][0]), "03" + hx(pts[3][0]), "02" + hx(pts[3][0])]  # (either prefix: the same entry)
    unc = ["04" + hx(pts[4][0]) + hx(pts[4][1]), "04" + hx(pts[5][0]) + hx(P - pts[5][1])]
    forty = ["751e76e8199196d454941c45d1b3a323f1433bd6", "7025b4efb3ff42eb4d6d71fab6b53b4f4967e3dd"]
    junk = ["05" + hx(pts[6][0]),                                   # 66 digits, not a key prefix
            "04" + hx(pts[7][0]) + hx((pts[7][1] + 1) % P),        # off the curve
            "04" + hx(pts[7][0]) + hx(pts[8][1]),                  # x and y of different points
            "05" + hx(pts[6][0]) + hx(pts[6][1]),                  # 130 digits, not 04
            "0x" + hx(pts[9][0]), "0x" + forty[0],                 # 0x-prefixed
            hx(pts[9][0])[:63], hx(pts[9][0]) + "0",                # 63 and 65 digits
            "02" + hx(pts[9][0])[:40] + "zz" + hx(pts[9][0])[42:],  # not hex beyond the leading 40
            "04" + hx(P) + hx(pts[4][1]),                           # x = p (not below p)
            "g" * 64]
    lines = [bare[0], forty[0], junk[0], comp[0], junk[1], unc[0], junk[2], bare[1], junk[3], comp[1], forty[1], junk[4], junk[5], unc[1],
             junk[6], comp[2], junk[7], junk[8], junk[9], junk[10]]
    text = "\n".join(lines) + "\n"
    with_x = {hx(pts[i][0])[:40] for i in (0, 1, 2, 3, 4, 5)}
    # the default rule: every full 40-character piece of a line that is clean hex is an entry
    default = set()
    for l in lines:
        for p in range(0, len(l) - 39, 40):
            if re.fullmatch(r"[0-9a-fA-F]{40}", l[p:p + 40]):
                default.add(l[p:p + 40].lower())
    ask = sorted(default | with_x)
    assert with_x != default
    for on, want in ((True, with_x), (False, default)):
        blf = str(tmp_path / ("l%d.blf" % on))
        pr = subprocess.run([cli, "blf-gen", "-n", "1000", "-o", blf] + (["-a", "x"] if on else []), input=text.encode(), capture_output=True,
                            timeout=120, env=env)
        assert pr.returncode == 0, pr.stderr
        assert b"added %d new items" % len(want) in pr.stdout, (on, pr.stdout)
        pr = subprocess.run([cli, "blf-check", "-f", blf] + ask, capture_output=True, text=True, timeout=120, env=env)
        found = {l.split()[0] for l in pr.stdout.splitlines() if l.endswith(" FOUND") and not l.endswith("NOT FOUND")}
        assert found == want, (on, pr.stdout)
    # a hash160 list given to a public-key search by mistake holds no entry
    lst = tmp_path / "p2pkh.txt"
    lst.write_text("\n".join(forty) + "\n")
    pr = subprocess.run([cli, "add", "-a", "x", "-f", str(lst), "-r", "8000:ffff"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60,
                        env=env)
    assert pr.returncode != 0 and "no hashes in filter file" in pr.stderr


def test_the_new_kernels_fit_168_registers_keep_scratch_out_of_their_loops_and_do_not_hash():
    """static, from the assembly the build keeps (tools/isa_mix.py: analyse_pub): each public-key kernel has at most 168 VGPRs and no scratch
    instruction in any loop below its launch loop (k_add_pub) / its round loops (k_mul_check_pub); the loop nest was seen; and the static
    per-key VALU count of k_add_pub<false> (the `which` loop body + half the table loop's own body + half the prefix loop, the figure
    tools/isa_mix.py gives every walk kernel) is below that of k_add for -a c from the same assembly less the 2 248 VALU lane-ops of one
    hash160: the hash is gone.  Figures of this build: 813 against 3 272 - 2 248 = 1 024."""
    import isa_mix
    now = isa_mix.analyse_pub(kept_assembly())
    assert set(now) == set(isa_mix.PUB_KERNELS) and len(now) == 3
    for label, a in now.items():
        print(label, a["registers"], {k: v for k, v in a.items() if k.startswith(("scratch", "window", "walk", "which", "per_key", "addr33", "table", "prefix", "image"))})
        assert a["registers"]["vgpr_count"] <= 168, (label, a["registers"])
        assert a["loops"] and a["scratch_below_top"] == 0, (label, a["loops"])
        if label == "mul -a x":
            assert a["scratch_in_round_loops"] == 0 and a["window_loop_mad64"] == 918, (label, a)
        else:
            assert any(l["depth"] >= 3 for l in a["loops"])  # launch > table > `which`: the loop nest was seen
    plain = now["-a x"]
    assert isa_mix.HASH160_VALU == 2248
    print("per-key VALU: -a x %.1f, -a c %.1f, -a c less hash160 %.1f" % (plain["per_key_valu"], plain["addr33_per_key_valu"], plain["addr33_less_hash160"]))
    assert 0 < plain["per_key_valu"] < plain["addr33_per_key_valu"] - 2248
    # no y of a walked point: one multiplication and one squaring in the `which` loop (81 + 9 x 2 and 45 + 9 x 2 + ... multiply-adds: fewer
    # than two multiplications' worth), against three and a half multiplications in k_add's
    assert plain["loops"] and max(l["mad64"] for l in plain["loops"] if l["depth"] == 3) < 2 * 99


class PubStandIn:
    """the surface engine.KeySearch needs of a device, with the GPU replaced by the yardstick: add_range / mul_batch report every key
    whose leading 20 bytes of x are listed (the list is the filter), verify_pub re-derives from the oracle's points"""
    corrupt = False

    def __init__(self, device=0, a33=True, a65=False, endo=False, ord_offs=0, pub=False):
        assert pub and not (a33 or a65)
        self.endo, self.offs, self.listed = endo, ord_offs, set()

    def close(self):
        pass

    def set_bloom(self, words):
        pass

    def set_list(self, hashes):
        self.listed = {tuple(int(v) for v in h) for h in hashes}

    def geometry(self):
        return 8, 256

    def _recs(self, items):
        from ecloop_amd import capi
        out = np.zeros(len(items), dtype=capi.FOUND_DTYPE)
        for r, (off, endo, h) in zip(out, items):
            r["key_offset"], r["endo"], r["compressed"], r["h160"] = off, endo, 5, h
        return out

    def add_range(self, start, nkeys, cap=4096):
        items = []
        for off in range(nkeys):
            k = (start + (off << self.offs)) % N
            for endo, h in (pub_ref.endo_images(k).items() if self.endo else [(0, pub_ref.h160_of(k))]):
                if h in self.listed:
                    items.append((off, endo, h))
        return self._recs(items[:cap]), len(items)

    def mul_batch(self, ks, cap=4096):
        items = [(i, 0, pub_ref.h160_of(k)) for i, k in enumerate(ks) if k % N and pub_ref.h160_of(k) in self.listed]
        return self._recs(items[:cap]), len(items)

    def verify_pub(self, ks):
        pts = [orc.point_of(k % N) for k in ks]
        x = np.array([[(p[0] >> (32 * (7 - j))) & 0xFFFFFFFF for j in range(8)] for p in pts], np.uint32).reshape(len(ks), 8)
        if PubStandIn.corrupt:
            x[0][4] ^= 1  # inside the 20 bytes a record holds
        return x, np.array([p[1] & 1 for p in pts], np.uint8), np.ones(len(ks), np.uint8)


def test_keysearch_pub_prints_the_compressed_key_and_a_mismatch_ends_the_run():
    """engine.KeySearch(pub=True) on a stand-in device: a pub record is verified against the leading 20 bytes of the re-derived x and then
    carries the whole key - its lines print the compressed key of the key that was walked (with the endomorphism: of the image's key);
    a re-derivation that does not match the record ends the run with the mismatch error, as for every other type"""
    from ecloop_amd import engine
    keys = [0x8123, 0x9001, 0xFFFE]
    listed = [keys[0], N - keys[1], pub_ref.calc_priv(keys[2], 2)]  # as itself, as its negative, as the lambda image
    hs = np.array(sorted(pub_ref.h160_of(k) for k in listed), np.uint32)
    flt = engine.Filter(np.zeros(64, np.uint64), hs)
    ks = engine.KeySearch(flt, pub=True, endo=True, device_cls=PubStandIn)
    assert ks.pub and not ks.a33
    ks.add_keys(0x8000, 0x8000)
    want = sorted([keys[0], keys[1], pub_ref.calc_priv(keys[2], 2)])
    assert sorted(r.pk for r in ks.found) == want
    assert sorted(r.stdout_line() for r in ks.found) == sorted(pub_ref.found_line(k) for k in want)
    assert sorted(r.line() for r in ks.found) == sorted("pub\t%s\t%064x" % (pub_ref.compressed(k), k) for k in want)
    assert {r.prefix for r in ks.found} <= {"02", "03"} and all(len(r.h160) == 8 for r in ks.found)
    m = engine.KeySearch(flt, pub=True, device_cls=PubStandIn)
    m.cmd_mul([5, keys[0], 0, 77])
    assert [r.stdout_line() for r in m.found] == [pub_ref.found_line(keys[0])]
    PubStandIn.corrupt = True
    try:
        bad = engine.KeySearch(flt, pub=True, device_cls=PubStandIn)
        with pytest.raises(engine.EclError, match="hash mismatch"):
            bad.add_keys(0x8000, 0x400)
    finally:
        PubStandIn.corrupt = False
