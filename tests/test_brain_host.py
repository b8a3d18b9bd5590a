"""`brain` without a GPU: the yardstick (tests/brain_ref.py: itertools.product) against the device's expansion compiled for the host
(csrc/gen.h through csrc/tools/gen_host.cpp, thread by thread as k_gen_lines runs it), the host program's own expansion
(gen_candidate_host of host/gen_plan.h), and engine.brain_candidate; the packed template and its validator; the mask and set parsers of
the host program and of engine.py; every refusal of the command; `brain -keys` against the yardstick and kdf_ref; the pins of the header
and the bindings; gen_host.cpp's own main under the sanitizers."""
import ctypes as C
import hashlib
import os
import re
import struct
import subprocess

import pytest

import brain_ref as R
import kdf_ref
from support import ROOT, cli, host_lib, host_program, run_program

# 65537 * 257 * 17 * 15 * 256^4 = (2^32 - 1) * 2^32: the largest T below 2^64 that few alternatives reach (2^64 - 59 is prime, and
# 2^64 - 1 has the factor 6700417, more than the 2^22 alternatives of a template)
WIDE_RADICES = [65537, 257, 17, 15, 256, 256, 256, 256]
WIDE_T = 0xFFFFFFFF00000000


def wide_positions():
    return [[b"%x" % a for a in range(r)] for r in WIDE_RADICES]


@pytest.fixture(scope="module")
def G(tmp_path_factory):
    lib = host_lib(tmp_path_factory, "gen_host.cpp")
    lib.gh_check.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint32), C.c_char_p]
    lib.gh_device_lines.argtypes = [C.c_char_p, C.c_size_t, C.c_ulonglong, C.c_uint32, C.c_char_p, C.POINTER(C.c_ulonglong)]
    lib.gh_device_lines.restype = C.c_uint32
    lib.gh_host_candidate.argtypes = [C.c_char_p, C.c_size_t, C.c_ulonglong, C.c_char_p]
    lib.gh_parse_mask.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t, C.c_char_p]
    lib.gh_parse_mask.restype = C.c_long
    lib.gh_threads_r.restype = C.c_uint32
    return lib


def check(G, blob):
    """-> (T, L) of an accepted blob, or the validator's reason"""
    T, L, why = C.c_ulonglong(), C.c_uint32(), C.create_string_buffer(160)
    return (T.value, L.value) if G.gh_check(blob, len(blob), C.byref(T), C.byref(L), why) == 0 else why.value.decode()


def device_lines(G, blob, first, m):
    """what a k_gen_lines launch writes for candidates first ... first + m - 1, cut out of its text by its line table; the table's
    offsets are the slots'"""
    _, L = check(G, blob)
    stride = max(4, (L + 3) // 4 * 4)
    text = C.create_string_buffer(m * stride + 8)
    lines = (C.c_ulonglong * m)()
    assert G.gh_device_lines(blob, len(blob), first, m, text, lines) == stride
    assert [l & 0xFFFFFFFF for l in lines] == [j * stride for j in range(m)]
    return [text.raw[j * stride: j * stride + (lines[j] >> 32)] for j in range(m)]


def host_candidates(G, blob, first, m):
    out = []
    buf = C.create_string_buffer(256)
    for i in range(first, first + m):
        n = G.gh_host_candidate(blob, len(blob), i, buf)
        assert n >= 0
        out.append(buf.raw[:n])
    return out


def agree(G, positions, windows):
    """the four expansions on every window (first, n)"""
    from ecloop_amd import engine
    blob = R.blob(positions)
    assert engine.brain_table(positions) == blob and check(G, blob)[0] == R.count(positions)
    for first, n in windows:
        want = R.window(positions, first, n)
        assert device_lines(G, blob, first, n) == want, (first, n)
        assert host_candidates(G, blob, first, n) == want, (first, n)
        assert [engine.brain_candidate(positions, first + j) for j in range(n)] == want, (first, n)


WORDS = [b"", b"a", b"bc", b"def", b"ghij", b"klmno", b"correct horse", b"x" * 255]
SMALL = {
    "a single position": [[b"alpha", b"be", b"", b"gamma!"]],
    "radix 1 between others": [[b"a", b"bb"], [b"-"], [b"0", b"1", b"2"], [b"_"], [b"x", b"yz"]],
    "radices 1 and 2 throughout": [[b"0", b"1"] if p % 2 == 0 else [b"."] for p in range(16)],
    "sixteen positions": [[b"<", b"", b">>>"] if p in (0, 15) else [b"%d" % p, b"%c%c" % (65 + p, 97 + p)] if p % 2 else [b"%c" % (97 + p)] for p in range(16)],
    "L = 1": [[b""], [b"a", b"", b"c"], [b""]],
    "words of mixed lengths": [WORDS[:7], [b" "], WORDS[:7]],
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_every_index_of_a_small_template_agrees_four_ways(G, name):
    positions = SMALL[name]
    T = R.count(positions)
    assert T <= 1 << 16
    assert R.candidates(positions) == R.window(positions, 0, T)  # the product itself against its digit form
    r = G.gh_threads_r()
    agree(G, positions, [(0, T), (1, T - 1), (T - 1, 1)] + [(first, min(r + 3, T - first)) for first in (1, r - 1, r + 1, 2 * r + 3) if first < T])


def test_the_longest_alternative_the_empty_one_and_the_longest_candidate(G):
    """a 255-byte word and a 0-byte one in one position; L = 256 from 255 + 1; words whose lengths are 0 ... 255 (the length is not the stride)"""
    agree(G, [[b"x" * 255, b""], [b"y", b""]], [(0, 4)])
    agree(G, [[b"q" * 250, b"r"], [b"123456", b""]], [(0, 4)])
    ramp = [bytes((i + j) % 251 + 1 for j in range(i)) for i in range(256)]
    agree(G, [ramp, [b"", b"!"]], [(0, 512), (3, 7)])


def test_indices_around_two_to_the_32_and_the_last_ones_of_a_template_near_two_to_the_64(G):
    positions = wide_positions()
    assert R.count(positions) == WIDE_T == (2 ** 32 - 1) << 32
    r = G.gh_threads_r()
    agree(G, positions, [((1 << 32) - 9, 20), ((1 << 32) + 1, r + 3), (WIDE_T - 21, 21), (WIDE_T - 1, 1), (0, 5), ((1 << 63) + 5, r + 3)])
    blob = R.blob(positions)
    buf = C.create_string_buffer(256)
    assert G.gh_host_candidate(blob, len(blob), WIDE_T, buf) == -1  # the first index outside


def test_a_run_of_r_plus_3_candidates_from_a_start_that_is_no_multiple_of_r(G):
    positions = [[b"ab", b"c", b"def"], [b"0", b"1"], [b"", b"xy", b"z", b"wwww"], [b"!"], [b"p", b"qq", b"r"]]
    r = G.gh_threads_r()
    T = R.count(positions)
    agree(G, positions, [(first, r + 3) for first in range(1, 2 * r + 2) if first % r and first + r + 3 <= T])


def test_the_blob_round_trip_and_every_malformed_field(G):
    from ecloop_amd import engine
    positions = [[b"pass"], [b"0", b"1", b"22"], [b"", b"!"]]
    blob = R.blob(positions)
    assert engine.brain_table(positions) == blob and engine.brain_positions(blob) == positions
    assert check(G, blob) == (6, 7)
    def patched(at, fmt, value):
        b = bytearray(blob)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)
    npos, nalt = 3, 6
    alt_at = 16 + 8 * npos
    bad = {
        "magic": patched(0, "<4s", b"GEX\0"), "zero": patched(6, "<B", 1), "npos 0": patched(4, "<B", 0), "npos 17": patched(4, "<B", 17),
        "nalt": patched(8, "<I", nalt + 1), "nalt 0": patched(8, "<I", 0), "pool_bytes": patched(12, "<I", 10), "pool above 2^28": patched(12, "<I", (1 << 28) + 1),
        "count 0": patched(16 + 8, "<I", 0), "count": patched(16 + 8, "<I", 2), "first": patched(16 + 8 + 4, "<I", 2),
        "alt off": patched(alt_at + 8 * 5, "<I", 9), "alt len": patched(alt_at + 8 * 3 + 4, "<I", 256), "alt outside": patched(alt_at + 8 * 3 + 4, "<I", 9),
        "nalt above 2^22": patched(8, "<I", (1 << 22) + 1),
        "short": blob[:-1], "long": blob + b"\0", "header only": blob[:12],
    }
    for name, b in bad.items():
        got = check(G, b)
        assert isinstance(got, str) and got, (name, got)
    assert "magic" in check(G, bad["magic"]) and "zero" in check(G, bad["zero"]) and "outside the pool" in check(G, bad["alt outside"])
    assert "2^22" in check(G, bad["nalt above 2^22"]) and "2^28" in check(G, bad["pool above 2^28"])
    assert "add up" in check(G, bad["count"]) and "add up" in check(G, bad["first"]) and "255" in check(G, bad["alt len"])
    # the limits: 17 positions cannot be written (npos is checked first); L = 257; T = 2^64 exactly and just below
    assert "256 bytes" in check(G, R.blob([[b"x" * 255], [b"yy"]]))
    assert check(G, R.blob([[b"x" * 255], [b"y"]])) == (1, 256)
    assert "2^64" in check(G, R.blob([[b"%x" % a for a in range(16)]] * 16))
    assert check(G, R.blob([[b"%x" % a for a in range(16)]] * 15 + [[b"%x" % a for a in range(15)]])) == (15 << 60, 16)
    with pytest.raises(ValueError, match="2\\^64"):
        engine.brain_count([[b"%x" % a for a in range(16)]] * 16)
    with pytest.raises(ValueError, match="256 bytes"):
        engine.brain_table([[b"x" * 255], [b"yy"]])
    with pytest.raises(ValueError):
        engine.brain_candidate(positions, 6)


def parse(G, mask, sets=()):
    """gh_parse_mask -> positions (through engine.brain_positions), or the parser's reason"""
    from ecloop_amd import engine
    arr = (C.c_char_p * 4)(*[(sets[k].encode("latin-1") if k < len(sets) and sets[k] is not None else None) for k in range(4)])
    blob, why = C.create_string_buffer(1 << 16), C.create_string_buffer(320)
    n = G.gh_parse_mask(mask.encode("latin-1"), arr, blob, len(blob), why)
    return engine.brain_positions(blob.raw[:n]) if n >= 0 else why.value.decode()


def test_the_mask_and_set_parsers_of_the_host_program_and_of_the_engine(G, tmp_path):
    from ecloop_amd import engine
    one = lambda s: [bytes([c]) for c in s]
    lower, upper, digits = bytes(range(97, 123)), bytes(range(65, 91)), b"0123456789"
    specials = bytes(c for c in range(32, 127) if not chr(c).isalnum())
    assert len(specials) == 33
    words = tmp_path / "words.txt"
    words.write_bytes(b"alpha\r\n\nbeta\n\r\nalpha\ngamma")
    cases = [
        ("pass?d?d", (), [[b"pass"], one(digits), one(digits)]),
        ("?l?u?h?s?a", (), [one(lower), one(upper), one(b"0123456789abcdef"), one(specials), one(lower + upper + digits + specials)]),
        ("a??b?1??", ("x?dy",), [[b"a?b"], one(b"x" + digits + b"y"), [b"?"]]),
        ("?1 ?2", ("@" + str(words), "@" + str(words)), [[b"alpha", b"beta", b"alpha", b"gamma"], [b" "], [b"alpha", b"beta", b"alpha", b"gamma"]]),
        ("?4?3x", (None, None, "??-", "ab"), [one(b"ab"), one(b"?-"), [b"x"]]),
        ("y" * 256, (), [[b"y" * 255], [b"y"]]),
    ]
    for mask, sets, want in cases:
        assert parse(G, mask, sets) == want, mask
        assert engine.parse_mask(mask, {k + 1: s for k, s in enumerate(sets) if s is not None}) == want, mask
    refused = [("?x", (), "unknown class ?x"), ("abc?", (), "unknown class"), ("?2", ("ab",), "?2 needs -2"), ("?d" * 17, (), "more than 16 positions"),
               ("?1", ("aba",), "twice"), ("?1", ("?da5",), "twice"), ("?1", ("?q",), "unknown class ?q"), ("?1", ("@" + str(tmp_path / "none"),), "cannot read"), ("", (), "empty")]
    for mask, sets, word in refused:
        assert word in parse(G, mask, sets), (mask, parse(G, mask, sets))
    for mask, custom in [("?x", None), ("?2", {1: "ab"}), ("?d" * 17, None), ("?1", {1: "aba"}), ("", None)]:
        with pytest.raises(ValueError):
            engine.parse_mask(mask, custom)


def test_the_harness_as_a_program_under_the_sanitizers(tmp_path):
    """gen_host.cpp's own main, built with ASan + UBSan and run directly: the table and the text live in heap blocks of exactly the sizes
    the library gives the device, so a gather behind the two spare words or a store outside a slot is a heap overflow"""
    pr = run_program(host_program(tmp_path, "gen_host.cpp", ["-O1"]), timeout=300)
    assert pr.returncode == 0 and pr.stdout.strip() == "ok", (pr.stdout, pr.stderr[-2000:])


def keys_of(cli, args):
    pr = subprocess.run([cli, "brain", "-keys"] + args, stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    assert pr.returncode == 0, pr.stderr
    return [tuple(l.split(b"\t")) for l in pr.stdout.split(b"\n") if l]


@pytest.mark.parametrize("kdf", ["sha256", "keccak", "sha3", "camp2"])
def test_brain_keys_is_the_yardstick_and_the_reference_digest(cli, tmp_path, kdf):
    words = tmp_path / "words.txt"
    words.write_bytes(b"correct\nhorse\r\nbattery\n\nstaple\nhorse\n")
    wl = [b"correct", b"horse", b"battery", b"staple", b"horse"]
    positions = [wl, [b" "], wl, [b"?"], [bytes([c]) for c in b"0123456789"]]
    T = R.count(positions)
    first, last = (0, T - 1) if kdf != "camp2" else (117, 118)  # (2031 permutations a line in Python)
    got = keys_of(cli, ["-mask", "?1 ?1???d", "-1", "@" + str(words), "-kdf", kdf, "-r", "%x:%x" % (first, last)])
    want = R.candidates(positions, first, last - first + 1)
    assert got == [(b"%x" % (first + j), w, kdf_ref.digest(kdf, w).hex().encode() if kdf != "sha256" else hashlib.sha256(w).hexdigest().encode()) for j, w in enumerate(want)]
    if kdf == "sha256":  # the default range is all of it; a wide template at its last indices
        assert keys_of(cli, ["-mask", "?1 ?1???d", "-1", "@" + str(words)]) == got
        wide = keys_of(cli, ["-mask", "?h?h?h?h?h?h?h?h?h?h?h?h?h?h?h?d", "-r", "9fffffffffffffff:9fffffffffffffff"])
        assert wide == [(b"9fffffffffffffff", b"fffffffffffffff9", hashlib.sha256(b"fffffffffffffff9").hexdigest().encode())]


def test_every_refusal_of_the_command_comes_before_a_gpu_is_looked_for(cli, tmp_path):
    lst = os.path.join(ROOT, "tests", "golden", "btc-puzzles-hash")
    long_words = tmp_path / "long.txt"
    long_words.write_bytes(b"x" * 130 + b"\n")
    m = ["-mask", "pass?d?d"]
    cases = [([], "brain needs a template: -mask"), (["-mask", "pass?x"], "unknown class ?x"), (["-mask", "a?3"], "?3 needs -3"), (["-mask", "?d" * 17], "more than 16 positions"),
             (["-mask", "?1?1", "-1", "@" + str(long_words)], "longer than 256 bytes"), (["-mask", "?h" * 16], "2^64 candidates or more"),
             (m + ["-r", "0:64"], "the template has 64 candidates"), (m + ["-r", "5:4"], "a is above b"), (m + ["-r", "zz"], "invalid -r"), (m + ["-r", "1:10000000000000000"], "invalid -r"),
             (m + ["-raw"], "-raw"), (m + ["-bin"], "-bin"), (m + ["-p", "1abc"], "-p 1abc"), (m + ["-k", "02" + "11" * 32], "-k 02"), (m + ["-path", "m/0"], "-path"),
             (m + ["-pass", "x"], "-pass x"), (m + ["-t", "2"], "-t 2"), (m + ["-kdf", "md5"], "invalid -kdf 'md5'"), (m + ["-1", "aa"], "twice"), (m + ["-q"], "quiet mode chosen without output file")]
    for extra, word in cases:
        pr = subprocess.run([cli, "brain", "-f", lst] + extra, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60)
        assert pr.returncode == 1 and pr.stdout == "" and word in pr.stderr, (extra, pr.stderr)
        assert "no MI355X GPU visible" not in pr.stderr, extra
    assert "brain" in subprocess.run([cli], capture_output=True, text=True, timeout=60).stdout


def test_the_bindings_constant_the_header_and_the_export_count():
    from ecloop_amd import capi
    assert capi.GEN == 0x20000 and len(capi.EXPORTS) == 45
    hdr = open(os.path.join(ROOT, "include", "ecloop_hip.h")).read()
    assert re.search(r"#define ECL_GEN 0x20000u\b", hdr) and "u32 count; u32 first;" in hdr
    assert capi.GEN & (capi.BIP39 | capi.KDF_CAMP2 | capi.MASK | capi.PREFIX | capi.HERD | capi.INSERT | capi.ORIGIN | capi.PUB | capi.TR | capi.ETH | capi.P2SH | 7) == 0
    with pytest.raises(ValueError):
        capi.Device(0, gen=True, bip39=True)
    with pytest.raises(ValueError):
        capi.Device(0, a33=False, eth=True, mask=True, gen=True)
