"""`brain` on the GPU (ECL_GEN): the records of ecl_hip_mul_batch_raw on a context that generates its lines against those of the same
context without the flag, fed the lines of tests/brain_ref.py - call shapes from one piece to several with the merged last one, first
indices odd, across 2^32 and up to the last candidate of a template near 2^64; candidate lengths at the hashes' block edges; every kdf and
address type; split calls and a changed template; coverage; the refusals of ecl_hip_open and of the call; the self-test; and the host
program end to end.  All-ones filter unless stated.  Every GPU-using subprocess runs under its own time limit."""
import ctypes as C
import hashlib
import os
import struct

import numpy as np
import pytest

import brain_ref as R
import kdf_ref
import mul_ref
import orc
from support import cli, run_cli
from walk_ref import canon, difference

pytestmark = pytest.mark.gpu
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
E_ARG, E_COVERAGE = -1, -8
LOWER = [bytes([c]) for c in range(97, 123)]
DIGITS = [bytes([c]) for c in b"0123456789"]
# 65537 * 257 * 17 * 15 * 256^4 = (2^32 - 1) * 2^32 = 0xFFFFFFFF00000000 (tests/test_brain_host.py: why not 2^64 - 59)
WIDE = [[b"%x" % a for a in range(r)] for r in (65537, 257, 17, 15, 256, 256, 256, 256)]
WIDE_T = 0xFFFFFFFF00000000


class Pair:
    """a generating context and the same context without the flag, both behind the all-ones filter"""

    def __init__(self, kdf=None, **kw):
        from ecloop_amd import Device
        self.kw = kw or dict(a33=True)
        self.per = sum(bool(self.kw.get(k)) for k in ("a33", "a65", "p2sh", "eth", "tr", "pub"))
        self.gen, self.plain = Device(0, kdf=kdf, gen=True, **self.kw), Device(0, kdf=kdf, **self.kw)
        self.gen.set_bloom(ONES), self.plain.set_bloom(ONES)

    def close(self):
        self.gen.close(), self.plain.close()

    def same(self, positions, first, n, lines=None):
        """the records of candidates first ... first + n - 1, generated, against those of the yardstick's lines, sent"""
        lines = R.window(positions, first, n) if lines is None else lines
        assert len(lines) == n
        got, total = self.gen.brain_batch(positions, first, n, cap=self.per * n + 8)
        want, total2 = self.plain.mul_batch_raw(lines, cap=self.per * n + 8)
        assert total == total2 == self.per * n
        assert difference(canon(got), canon(want)) == ""
        return got


@pytest.fixture(scope="module")
def sha():
    p = Pair()
    yield p
    p.close()


@pytest.mark.parametrize("first,n", [(0, 5000), (1, (1 << 17) + 3), (77777, 3 * (1 << 18) + 7)])
def test_one_piece_two_pieces_and_several_with_the_merged_last_one(sha, first, n):
    positions = [LOWER, LOWER, [b"-"], LOWER, LOWER, DIGITS]  # 4 569 760 candidates of 6 bytes
    if n > 1 << 19:
        assert len(mul_ref.pieces(n)) >= 3
    sha.same(positions, first, n, lines=R.candidates(positions, first, n))


def test_first_indices_across_two_to_the_32_and_up_to_the_last_candidate_near_two_to_the_64(sha):
    assert R.count(WIDE) == WIDE_T
    blob = R.blob(WIDE)
    for first, n in (((1 << 32) - 2501, 5000), (WIDE_T - 4999, 4999), ((1 << 63) + 12345, 300)):
        sha.same(blob, first, n, lines=R.window(WIDE, first, n))
    before = sha.gen.coverage()
    for first, n in ((WIDE_T - 4999, 5000), (WIDE_T, 1), ((1 << 64) - 1, 2)):  # first + n > T
        with pytest.raises(Exception) as e:
            sha.gen.brain_batch(blob, first, n, cap=16)
        assert e.value.code == E_ARG and "passes the template's number of candidates" in str(e.value)
    assert sha.gen.coverage() == before  # nothing was launched
    sha.same(blob, WIDE_T - 1, 1, lines=R.window(WIDE, WIDE_T - 1, 1))


def exact(length):
    """100 candidates of exactly `length` bytes"""
    return [[bytes((7 * i) % 95 + 32 for i in range(length - 2))], DIGITS, DIGITS]


EDGES = {"sha256": (55, 56, 63, 64, 65), "keccak": (135, 136, 137), "sha3": (135, 136, 137)}


@pytest.mark.parametrize("kdf", ["sha256", "keccak", "sha3"])
def test_every_kdf_at_its_block_edges_and_at_the_templates_extremes(kdf):
    ramp = [bytes((i + j) % 251 + 1 for j in range(i)) for i in range(0, 253, 3)]  # words of 0, 3, ... 252 bytes: the length is not the stride
    p = Pair(kdf=None if kdf == "sha256" else kdf)
    try:
        for length in EDGES[kdf]:
            got = p.same(exact(length), 0, 100)
            assert len(got) == 100
        p.same([[b"a", b"", b"c"]], 0, 3)                                   # L = 1, and the empty candidate
        p.same([[b"x" * 255, b""], [b"y", b"z"]], 0, 4)                     # L = 256; a 0-byte alternative beside the longest
        p.same([ramp, [b"", b"!"], DIGITS], 3, len(ramp) * 20 - 3)
        p.same([LOWER, LOWER, LOWER, DIGITS], 9, 5000)
        # three candidates as literals: the record is the oracle's hash160 of the digest's key
        positions = [[b"pass"], DIGITS, DIGITS, DIGITS, DIGITS]
        got, _ = p.gen.brain_batch(positions, 40, 10000 - 40, cap=10000)
        by_offset = {int(r["key_offset"]): r for r in got}
        for index, phrase in ((42, b"pass0042"), (9999, b"pass9999"), (40, b"pass0040")):
            k = int.from_bytes(hashlib.sha256(phrase).digest() if kdf == "sha256" else kdf_ref.digest(kdf, phrase), "big") % orc.N
            assert list(by_offset[index - 40]["h160"]) == orc.hash160(*orc.point_of(k), True), phrase
    finally:
        p.close()


def test_camp2_on_256_candidates():
    p = Pair(kdf="camp2")
    try:
        p.same([[b"ether"], [b"camp", b"", b"wallet "], LOWER, DIGITS], 300, 256)
    finally:
        p.close()


@pytest.mark.parametrize("letters", ["c", "u", "cu", "s", "e", "t", "x"])
def test_every_address_type(letters):
    positions = [[b"correct", b"horse", b"battery", b"staple", b""], [b" "], LOWER, LOWER, DIGITS]
    p = Pair(**mul_ref.CONTEXTS[letters][1])
    try:
        assert p.per == len(letters)
        got = p.same(positions, 12345, 5000, lines=R.candidates(positions, 12345, 5000))
        if letters in ("c", "u", "cu"):
            by = {(int(r["key_offset"]), int(r["compressed"])): r for r in got}
            for index, phrase in ((12345, b"horse vm5"), (12346, b"horse vm6"), (17344, b"battery os4")):
                assert R.candidate(positions, index) == phrase
                k = int.from_bytes(hashlib.sha256(phrase).digest(), "big") % orc.N
                for comp in ([1] if letters == "c" else [0] if letters == "u" else [0, 1]):
                    assert list(by[(index - 12345, comp)]["h160"]) == orc.hash160(*orc.point_of(k), bool(comp)), (phrase, comp)
    finally:
        p.close()


def test_two_calls_are_one_and_a_changed_template_is_sent_again(sha):
    one = [LOWER, DIGITS, LOWER, [b"!", b"?", b""]]
    two = [DIGITS, DIGITS, [b"-"], LOWER, LOWER]  # other counts, other bytes, a blob of another length
    a, n1, n2 = 1001, 3000, 2500
    whole, _ = sha.gen.brain_batch(one, a, n1 + n2, cap=n1 + n2)
    part1, _ = sha.gen.brain_batch(one, a, n1, cap=n1)
    part2, _ = sha.gen.brain_batch(one, a + n1, n2, cap=n2)
    part2 = part2.copy()
    part2["key_offset"] += n1
    assert difference(canon(np.concatenate([part1, part2])), canon(whole)) == ""
    sha.same(two, 5, 4000)
    sha.same(one, a, n1)   # the first template again: the context held the second
    three = [list(p) for p in one]
    three[3] = [b"!", b"?", b"_"]  # the same length, one byte of the pool differs
    sha.same(three, a, n1)


def test_a_launch_that_runs_short_fails_the_coverage_check(sha):
    from ecloop_amd import capi
    positions = [LOWER, LOWER, DIGITS]
    sha.gen.diag_drop_round()
    with pytest.raises(capi.EclError) as e:
        sha.gen.brain_batch(positions, 0, 6000, cap=6000)
    assert e.value.code == E_COVERAGE
    sha.same(positions, 0, 6000)  # the context goes on


def test_the_flag_opens_beside_every_mul_context_and_nowhere_else():
    from ecloop_amd import capi
    lib = capi.load()
    A33, A65, P2SH, ENDO, GEN = capi.ADDR33, capi.ADDR65, capi.P2SH, capi.ENDO, capi.GEN
    bases = [A33, A65 | P2SH, A33 | A65 | P2SH | ENDO, capi.ETH, capi.ETH | ENDO, capi.TR, capi.PUB, capi.PUB | ENDO]
    for base in bases:
        for kdf in (0, capi.KDF_KECCAK, capi.KDF_SHA3, capi.KDF_CAMP2):
            h = C.c_void_p()
            assert lib.ecl_hip_open(C.byref(h), 0, base | kdf | GEN, 0) == 0, (base, kdf)
            lib.ecl_hip_close(h)
    refused = [capi.PUB | capi.ORIGIN, capi.PUB | capi.INSERT, capi.PUB | capi.HERD, A33 | capi.PREFIX, capi.ETH | capi.MASK, A33 | capi.BIP39]
    for base in refused:
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, base, 0) == 0, base  # valid without the flag ...
        lib.ecl_hip_close(h)
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, base | GEN, 0) == E_ARG, base  # ... and ECL_E_ARG with it
    for base in (0, ENDO, capi.ETH | A33, capi.TR | ENDO, 8, 32, capi.KDF_KECCAK):  # the flag is no type: alone, or beside a refused set, it opens nothing
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, base | GEN, 0) == E_ARG, base


@pytest.mark.parametrize("base", ["cu", "e", "t"])
def test_the_selftest_of_a_generating_context(base):
    from ecloop_amd import Device
    for kdf in (None, "keccak"):
        d = Device(0, kdf=kdf, gen=True, **mul_ref.CONTEXTS[base][1])
        try:
            d.selftest()
        finally:
            d.close()


def test_a_malformed_template_is_refused_with_a_message_and_nothing_is_launched(sha):
    positions = [[b"pass"], [b"0", b"1", b"22"], [b"", b"!"]]
    blob = R.blob(positions)
    def patched(at, fmt, value):
        b = bytearray(blob)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)
    alt_at = 16 + 8 * 3
    bad = [(patched(0, "<4s", b"GEX\0"), "magic"), (patched(7, "<B", 1), "zero"), (patched(4, "<B", 17), "16 positions"), (patched(8, "<I", 7), "length"),
           (patched(16 + 8, "<I", 2), "add up"), (patched(16 + 8 + 4, "<I", 2), "add up"), (patched(16, "<I", 0), "no alternative"),
           (patched(alt_at + 8 * 3 + 4, "<I", 9), "outside the pool"), (patched(alt_at + 8 * 5, "<I", 9), "outside the pool"), (patched(alt_at + 4, "<I", 256), "255"),
           (blob[:-1], "length"), (blob + b"\0", "length"), (blob[:10], "header"), (R.blob([[b"x" * 255], [b"yy"]]), "256 bytes"),
           (R.blob([[b"%x" % a for a in range(16)]] * 16), "2^64")]
    before = sha.gen.coverage()
    for b, word in bad:
        with pytest.raises(Exception) as e:
            sha.gen.brain_batch(b, 0, 1, cap=4)
        assert e.value.code == E_ARG and word in str(e.value), (word, str(e.value))
    assert sha.gen.coverage() == before
    sha.same(positions, 0, 6)


def test_add_range_and_mul_batch_are_those_of_the_context_without_the_flag(sha):
    import random
    rnd = random.Random(2 ** 17)
    ks = [rnd.getrandbits(256) for _ in range(997)] + [0, orc.N, orc.N + 5]
    a, na = sha.gen.add_range(0x123456789, 1 << 16, cap=1 << 16)
    b, nb = sha.plain.add_range(0x123456789, 1 << 16, cap=1 << 16)
    assert na == nb == 1 << 16 and difference(canon(a), canon(b)) == ""
    a, na = sha.gen.mul_batch(ks, cap=1000)
    b, nb = sha.plain.mul_batch(ks, cap=1000)
    assert na == nb == 998 and difference(canon(a), canon(b)) == ""


def test_engine_cmd_brain_finds_the_planted_phrase_and_counts_its_range(tmp_path):
    from ecloop_amd.engine import KeySearch, load_filter
    k = int.from_bytes(hashlib.sha256(b"pass0042").digest(), "big")
    h = orc.hex160(orc.hash160(*orc.point_of(k % orc.N), True))
    lst = tmp_path / "list.txt"
    lst.write_text(h + "\n")
    ks = KeySearch(load_filter(str(lst)), device=0, gen=True)
    try:
        found = ks.cmd_brain("pass?d?d?d?d", first=0x20, last=0x270e)
        assert [r.line() for r in found] == ["addr33\t%s\t%064x\t2a\tpass0042" % (h, k)] and ks.k_checked == 0x270e - 0x20 + 1
        assert ks.cmd_brain("pass?1", {1: "?d"}, first=0, last=9) == found  # nothing more under another template
    finally:
        ks.close()


# ------------------------------------------------------------------------------------------------ the host program

def mul_raw_fields(cli, phrases, extra=()):
    """the first three fields of the lines `mul -raw` prints for the phrases on stdin (label, hash, key)"""
    r = run_cli(cli, ["mul", "-raw", *extra], stdin="".join(p + "\n" for p in phrases), hard_limit=240)
    return sorted(" ".join(l.split()[:4]) for l in r.found)


def test_cli_brain_finds_the_two_planted_phrases_of_a_mask(cli, tmp_path):
    want = []
    for phrase in (b"pass0042", b"pass9999"):
        k = int.from_bytes(hashlib.sha256(phrase).digest(), "big")
        want.append((orc.hex160(orc.hash160(*orc.point_of(k % orc.N), True)), k, phrase.decode()))
    lst = tmp_path / "list.txt"
    lst.write_text("".join(h + "\n" for h, _, _ in want))
    r = run_cli(cli, ["brain", "-f", str(lst), "-mask", "pass?d?d?d?d"], hard_limit=240)
    assert r.found == sorted("addr33: %s <- %064x %x %s" % (h, k, int(p[4:]), p) for h, k, p in want), r.stdout
    assert "index: 270f / 2710" in r.status, r.status  # the index reached and T
    assert sorted(" ".join(l.split()[:4]) for l in r.found) == mul_raw_fields(cli, ["pass0042", "pass9999"], ["-f", str(lst)])
    out = tmp_path / "found.txt"
    r = run_cli(cli, ["brain", "-f", str(lst), "-mask", "pass?d?d?d?d", "-r", "2b:270e"], out=str(out), hard_limit=240)  # 0x2a = 42 and 0x270f = 9999 are cut off
    assert r.lines == [] and "index: 270e / 2710" in r.status
    r = run_cli(cli, ["brain", "-f", str(lst), "-mask", "pass?d?d?d?d", "-r", "2a:270e"], out=str(out), hard_limit=240)
    assert r.lines == ["addr33\t%s\t%064x\t2a\tpass0042" % (want[0][0], want[0][1])]


def test_cli_brain_two_word_lists_keccak_eth_and_a_range(cli, tmp_path):
    import eth_ref
    words = [b"w%03d" % i for i in range(100)] + [b"correct", b"horse", b"correct"]  # a duplicate word: duplicate candidates
    wl = tmp_path / "words.txt"
    wl.write_bytes(b"\n".join(words) + b"\n")
    positions = [words, [b" "], words]
    planted = {i: R.candidate(positions, i) for i in (100 * 103 + 101, 102 * 103 + 101, 5 * 103 + 7)}
    assert planted[100 * 103 + 101] == planted[102 * 103 + 101] == b"correct horse" and planted[5 * 103 + 7] == b"w005 w007"
    def line(i):
        k = kdf_ref.scalar("keccak", planted[i])
        return "eth: %s <- %064x %x %s" % (eth_ref.eth_hex(*orc.point_of(k % orc.N)), k, i, planted[i].decode())
    lst = tmp_path / "list.txt"
    lst.write_text("".join(sorted({"0x" + line(i).split()[1] + "\n" for i in planted})))
    args = ["brain", "-f", str(lst), "-a", "e", "-kdf", "keccak", "-mask", "?1 ?2", "-1", "@" + str(wl), "-2", "@" + str(wl)]
    r = run_cli(cli, args, hard_limit=240)
    assert r.found == sorted(line(i) for i in planted), r.stdout
    assert sorted(" ".join(l.split()[:4]) for l in r.found if "w005" in l) == mul_raw_fields(cli, ["w005 w007"], ["-kdf", "keccak", "-a", "e", "-f", str(lst)])
    r = run_cli(cli, args + ["-r", "0:%x" % (102 * 103 + 100)], hard_limit=240)  # the second "correct horse" is cut off
    assert r.found == sorted(line(i) for i in (100 * 103 + 101, 5 * 103 + 7)), r.stdout
    r = run_cli(cli, [a if a != "keccak" else "sha3" for a in args], hard_limit=240)  # the same phrases under SHA3-256 are other keys
    assert r.found == [], r.stdout


def test_cli_brain_stops_when_the_hosts_phrase_disagrees_with_the_devices(cli, tmp_path):
    k = int.from_bytes(hashlib.sha256(b"pass0042").digest(), "big")
    lst = tmp_path / "list.txt"
    lst.write_text(orc.hex160(orc.hash160(*orc.point_of(k % orc.N), True)) + "\n")
    args = ["brain", "-f", str(lst), "-mask", "pass?d?d?d?d"]
    r = run_cli(cli, args, env={"ECLOOP_HIP_TEST_BRAIN_DISAGREE": "1"}, hard_limit=240, check=False)
    assert r.returncode == 1 and "hash mismatch" in r.stderr and r.found == [] and " <- " not in r.stdout, r.stderr[-2000:]
    assert len(run_cli(cli, args, hard_limit=240).found) == 1
