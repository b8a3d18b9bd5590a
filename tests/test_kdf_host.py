"""`mul -raw -kdf` (Keccak-256, SHA3-256, the 2031-fold Keccak-256 of ethercamp) without a GPU: the reference (tests/kdf_ref.py) pinned
to hashlib and the known answers; the line hashing of the device header kdf.h compiled for the host (csrc/tools/kdf_host.cpp) against it
at every length and start alignment, with the text ending on the last line's last byte, and its flag for a line outside the text; the
host program's own Keccak through `parse -raw -kdf`, `-kdf sha256` against plain `-raw`, the three refusals; the binding's constants, the
export count and the header; engine.kdf_digest; and KeySearch(kdf=).cmd_mul_raw over a stand-in device built on the oracle."""
import ctypes as C
import hashlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

import kdf_ref
import orc
from fake_device import FakeDevice
from support import ROOT, cli, host_lib, host_program, run_program

LENGTHS = list(range(0, 301)) + [407, 408, 409, 1000, 4000]
KDF_ID = {"keccak": 1, "sha3": 2, "camp2": 3}


def test_the_reference_is_sha3_with_another_pad_byte_and_gives_the_known_answers():
    assert kdf_ref.self_check()
    rnd = random.Random(136)
    for n in (0, 1, 134, 135, 136, 137, 271, 272, 273, 4000):
        msg = bytes(rnd.randrange(256) for _ in range(n))
        assert kdf_ref.digest("sha3", msg) == hashlib.sha3_256(msg).digest(), n
        assert kdf_ref.digest("sha256", msg) == hashlib.sha256(msg).digest(), n
    import eth_ref
    assert kdf_ref.digest("keccak", b"") == eth_ref.keccak256(b"") and kdf_ref.digest("keccak", b"abc" * 99) == eth_ref.keccak256(b"abc" * 99)


@pytest.fixture(scope="module")
def K(tmp_path_factory):
    lib = host_lib(tmp_path_factory, "kdf_host.cpp")
    lib.kh_lines.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return lib


def device_digests(K, name, blob, table, have=None):
    """the kernel body over the table (start | length << 32) -> (digests as bytes, the two flags).  The text is copied into a buffer
    of the size the library gives it - the bytes, rounded up to words, and two spare words; nothing here would notice a read behind
    it: that is what test_kdf_h_as_a_program_under_the_sanitizers is for."""
    words = (len(blob) + 3) // 4 + 2
    text = np.zeros(words * 4, np.uint8)
    text[: len(blob)] = np.frombuffer(blob, np.uint8)
    t = np.array(table, dtype=np.uint64)
    out = np.zeros((len(t), 8), np.uint32)
    bad = np.zeros(2, np.uint32)
    K.kh_lines(text.ctypes.data, len(blob), len(blob) if have is None else have, t.ctypes.data, len(t), KDF_ID[name], out.ctypes.data, bad.ctypes.data)
    return [b"".join(int(w).to_bytes(4, "big") for w in row[::-1]) for row in out], [int(v) for v in bad]


def packed(lines, lead=0):
    """lines back to back behind `lead` bytes -> (text, table)"""
    table, at = [], lead
    for l in lines:
        table.append(at | (len(l) << 32))
        at += len(l)
    return b"\xA5" * lead + b"".join(lines), table


@pytest.mark.parametrize("name", ["keccak", "sha3"])
def test_kdf_h_absorbs_every_length_at_every_alignment(K, name):
    rnd = random.Random(1600)
    lines = [bytes(rnd.randrange(256) for _ in range(n)) for n in LENGTHS]
    want = [kdf_ref.digest(name, l) for l in lines]
    seen = set()
    for lead in range(4):  # every line at every start alignment; back to back, so the lengths shift the alignments too
        blob, table = packed(lines, lead)
        seen |= {(t & 3, (t >> 32) % 136 in (0, 135)) for t in table}
        got, bad = device_digests(K, name, blob, table)
        assert bad == [0, 0] and got == want, lead
        assert (table[-1] & 0xFFFFFFFF) + (table[-1] >> 32) == len(blob)  # the last line ends on the text's last byte
    assert {a for a, _ in seen} == {0, 1, 2, 3}
    # ... and a short last line, so that the word that holds the text's end is a partial one at each alignment
    for tail in (b"", b"x", b"xy", b"xyz", b"wxyz", b"vwxyz"):
        for lead in range(4):
            blob, table = packed([b"abc", tail], lead)
            got, bad = device_digests(K, name, blob, table)
            assert bad == [0, 0] and got == [kdf_ref.digest(name, b"abc"), kdf_ref.digest(name, tail)], (tail, lead)
    for (n, line), hexd in kdf_ref.KNOWN.items():
        if n == name:
            assert device_digests(K, name, line, [len(line) << 32])[0][0].hex() == hexd


def test_kdf_h_camp2_on_eight_lines(K):
    rnd = random.Random(2031)
    lines = [b"", b"abc", b"password"] + [bytes(rnd.randrange(256) for _ in range(n)) for n in (1, 31, 135, 136, 300)]
    blob, table = packed(lines, 1)
    got, bad = device_digests(K, "camp2", blob, table)
    assert bad == [0, 0] and got == [kdf_ref.digest("camp2", l) for l in lines]
    assert [g.hex() for g in got[:3]] == [kdf_ref.KNOWN["camp2", l] for l in (b"", b"abc", b"password")]


def test_kdf_h_as_a_program_under_the_sanitizers(tmp_path):
    """kdf_host.cpp's own main, built with ASan + UBSan and run directly: the known answers at the four alignments; every length 0..300, 407,
    408, 409, 1000, 4000 as the last line of a heap block that ends with the two spare words (a gather that read behind them is a heap
    overflow; a shift by 32 in the masks is undefined behaviour); both flags"""
    pr = run_program(host_program(tmp_path, "kdf_host.cpp", ["-O1", "-g"]), timeout=300)
    assert pr.returncode == 0 and pr.stdout.strip() == "ok", (pr.stdout, pr.stderr[-2000:])


@pytest.mark.parametrize("name", ["keccak", "sha3", "camp2"])
def test_kdf_h_flags_a_line_outside_the_text_and_a_line_that_is_not_there_yet(K, name):
    blob = b"0123456789"
    got, bad = device_digests(K, name, blob, [0 | (4 << 32), 8 | (3 << 32)])  # the second line ends one byte past the text
    assert bad == [1, 0] and got[0] == kdf_ref.digest(name, b"0123")
    got, bad = device_digests(K, name, blob, [0 | (4 << 32), 6 | (4 << 32)], have=8)  # inside the text, behind what is on the device
    assert bad == [0, 1] and got[0] == kdf_ref.digest(name, b"0123")
    got, bad = device_digests(K, name, blob, [6 | (4 << 32), 0xFFFFFFFF | (0xFFFFFFFF << 32)])  # start + length wraps 32 bits
    assert bad == [1, 0] and got[0] == kdf_ref.digest(name, b"6789")


# ---------------------------------------------------------------------------------------------------------------- the host program
def parse(cli, data, *flags):
    pr = subprocess.run([cli, "parse", "-raw"] + list(flags), input=data, capture_output=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    return pr.stdout.decode().split()


@pytest.mark.parametrize("name", ["keccak", "sha3"])
def test_parse_prints_the_digests_of_the_reference(cli, name):
    rnd = random.Random(17)
    alphabet = "abcdefghijklmnopqrstuvwxyz0123456789 !"
    lens = [1, 2, 3, 31, 32, 33, 134, 135, 136, 137, 138, 270, 271, 272, 273, 274, 407, 408, 409, 1000]
    words = ["".join(rnd.choice(alphabet) for _ in range(n)) for n in lens]  # (within a line's 1024 bytes: longer ones are cut into pieces)
    assert parse(cli, ("\n".join(words) + "\n").encode(), "-kdf", name) == [kdf_ref.digest(name, w.encode()).hex() for w in words]


def test_parse_camp2_known_answers(cli):
    """the three known answers; the empty phrase cannot be a line of the input (the reader lists non-empty lines only, as for SHA-256): it
    is dropped here, and its answer is checked where a line table can hold it (kdf.h above, the device in tests/test_gpu_kdf.py)"""
    assert parse(cli, b"\nabc\npassword\n", "-kdf", "camp2") == [kdf_ref.KNOWN["camp2", b"abc"], kdf_ref.KNOWN["camp2", b"password"]]
    assert parse(cli, b"\nabc\n", "-kdf", "keccak") == [kdf_ref.KNOWN["keccak", b"abc"]]
    assert parse(cli, b"abc\n", "-kdf", "sha3") == [kdf_ref.KNOWN["sha3", b"abc"]]
    assert kdf_ref.digest("camp2", b"").hex() == kdf_ref.KNOWN["camp2", b""]


def test_kdf_sha256_is_plain_raw_and_long_lines_are_cut_alike(cli):
    rnd = random.Random(4)
    words = ["".join(rnd.choice("abcdefghijklmnop ") for _ in range(n)) for n in list(range(1, 150)) + [1023, 1024, 1025, 3000]]
    data = ("\n".join(words) + "\r\n").encode()
    plain = parse(cli, data)
    assert parse(cli, data, "-kdf", "sha256") == plain and len(plain) > len(words)  # (the lines past 1024 bytes came out as pieces)
    # the KDF sees what SHA-256 sees: a line longer than 1024 bytes goes on as pieces of 1024, and every hash gets the same pieces
    pieces = [w[i: i + 1024] for w in words for i in range(0, len(w), 1024)]
    assert [hashlib.sha256(p.encode()).hexdigest() for p in pieces] == plain
    for name in ("keccak", "sha3"):
        assert parse(cli, data, "-kdf", name) == [kdf_ref.digest(name, p.encode()).hex() for p in pieces], name


def test_the_three_refusals_name_the_option(cli):
    def refused(args, data=b"abc\n"):
        pr = subprocess.run([cli] + args, input=data, capture_output=True, text=False, timeout=60)
        assert pr.returncode != 0 and b"-kdf" in pr.stderr, (args, pr.stderr)
        return pr.stderr.decode()
    for args in (["mul", "-kdf", "keccak", "-f", "/nonexistent"], ["add", "-kdf", "keccak", "-raw", "-f", "/nonexistent", "-r", "8000:ffff"],
                 ["rnd", "-kdf", "camp2", "-f", "/nonexistent"], ["parse", "-kdf", "sha3"]):
        assert "mul -raw" in refused(args)  # -kdf without mul -raw: refused before the filter is opened or a GPU is looked for
    assert "-bin" in refused(["mul", "-raw", "-bin", "-kdf", "keccak", "-f", "/nonexistent"])
    assert "-bin" in refused(["parse", "-raw", "-bin", "-kdf", "sha3"])
    msg = refused(["mul", "-raw", "-kdf", "keccak256", "-f", "/nonexistent"])
    assert all(n in msg for n in kdf_ref.NAMES) and "keccak256" in msg
    out = subprocess.run([cli], capture_output=True, text=True, timeout=60).stdout
    line = [l for l in out.splitlines() if l.strip().startswith("-kdf ")]
    assert len(line) == 1 and all(n in line[0] for n in kdf_ref.NAMES), out


# ---------------------------------------------------------------------------------------------------------------- binding and engine
def test_binding_constants_export_count_and_header():
    from ecloop_amd import capi
    assert (capi.KDF_KECCAK, capi.KDF_SHA3, capi.KDF_CAMP2) == (0x4000, 0x8000, 0xC000) and capi.KDF_CAMP2 == capi.KDF_KECCAK | capi.KDF_SHA3
    assert len(capi.EXPORTS) == 45 and len(set(capi.EXPORTS)) == 45
    header = open(os.path.join(ROOT, "include", "ecloop_hip.h")).read()
    for name, value in (("ECL_KDF_KECCAK", "0x4000u"), ("ECL_KDF_SHA3", "0x8000u"), ("ECL_KDF_CAMP2", "0xC000u")):
        assert re.search(r"#define %s %s\b" % (name, value), header), name
        assert len(re.findall(r"\b%s\b" % name, header)) >= 3, name  # defined, and described in the flags' comment
    assert "exactly the 45 ecl_hip_* functions" in header and "2031" in header
    assert len(set(re.findall(r"^(?:int|void|void \*|const char \*) ?(ecl_hip_\w+)\(", header, re.M))) == 45  # no new declaration
    from ecloop_amd.build import build_library
    nm = subprocess.run(["nm", "-D", "--defined-only", build_library()], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in nm.splitlines() if l.split()[1:2] == ["T"]) == sorted(capi.EXPORTS)  # the exports map's 45, nothing else
    for bad in (dict(prefix=True), dict(a33=False, eth=True, mask=True), dict(a33=False, pub=True, origin=True), dict(a33=False, pub=True, insert=True),
                dict(a33=False, pub=True, herd=True)):
        with pytest.raises(ValueError):
            capi.Device(0, kdf="keccak", **bad)  # (before the library is asked)
    with pytest.raises(ValueError):
        capi.Device(0, kdf="md5")


def test_engine_kdf_digest_against_the_reference():
    from ecloop_amd import engine
    rnd = random.Random(55)
    assert engine.KDF_NAMES == kdf_ref.NAMES
    for n in list(range(0, 140, 7)) + [134, 135, 136, 137, 271, 272, 273, 1000]:
        msg = bytes(rnd.randrange(256) for _ in range(n))
        for name in ("sha256", "keccak", "sha3"):
            assert engine.kdf_digest(name, msg) == kdf_ref.digest(name, msg), (name, n)
    for (name, line), hexd in kdf_ref.KNOWN.items():
        assert engine.kdf_digest(name, line).hex() == hexd, (name, line)
    with pytest.raises(ValueError):
        engine.kdf_digest("md5", b"")
    import ast
    tree = ast.parse(open(engine.__file__).read())
    mods = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names} | {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert not any(m and ("kdf_ref" in m or "eth_ref" in m or m.startswith("tests")) for m in mods)  # the engine stands without tests/


class FakeKdfDevice(FakeDevice):
    """the stand-in with a `mul -raw`: the digests of the reference, the oracle's hashes, the filter that was set"""
    opened = []
    corrupt = False

    def __init__(self, device=0, a33=True, a65=False, endo=False, ord_offs=0, kdf=None):
        super().__init__(device, a33=a33, a65=a65, endo=endo, ord_offs=ord_offs)
        self.kdf = kdf
        FakeKdfDevice.opened.append(kdf)

    def mul_batch_raw(self, lines, cap=4096):
        from ecloop_amd import capi
        flt = orc.OrcFilter(bloom_words=self.words)
        recs = []
        for i, l in enumerate(lines):
            k = kdf_ref.scalar(self.kdf or "sha256", l) % orc.N
            if FakeKdfDevice.corrupt:
                k ^= 1  # a device whose hash disagrees with the engine's
            x, y = orc.point_of(k)
            for comp, on in ((1, self.a33), (0, self.a65)):
                h = orc.hash160(x, y, bool(comp))
                if on and flt.check(h):
                    recs.append((i, h, 0, comp))
        arr = np.zeros(len(recs), dtype=capi.FOUND_DTYPE)
        for j, (off, h, e, c) in enumerate(recs):
            arr[j]["key_offset"], arr[j]["h160"], arr[j]["endo"], arr[j]["compressed"] = off, h, e, c
        self.kept = arr[: max(cap, self.keep_min)]
        return arr[:cap].copy(), len(recs)


@pytest.mark.parametrize("name", [None, "sha256", "keccak", "sha3", "camp2"])
def test_keysearch_cmd_mul_raw_reports_the_planted_lines_with_their_digests_as_keys(name):
    from ecloop_amd import engine
    rnd = random.Random(8)
    n = 5 if name == "camp2" else 300  # (a camp2 digest in plain Python takes half a second)
    lines = [bytes(rnd.randrange(32, 127) for _ in range(rnd.randrange(1, 60))) for _ in range(n)]
    planted = [1, n // 2, n - 1]
    keys = {i: kdf_ref.scalar(name or "sha256", lines[i]) for i in planted}
    hashes = sorted(orc.hash160(*orc.point_of(keys[i] % orc.N), True) for i in planted)
    flt = engine.Filter(np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64), np.array(hashes, dtype=np.uint32))
    FakeKdfDevice.opened, FakeKdfDevice.corrupt = [], False
    ks = engine.KeySearch(flt, device_cls=FakeKdfDevice, kdf=name)
    found = ks.cmd_mul_raw(lines)
    assert FakeKdfDevice.opened == [None if name in (None, "sha256") else name]
    assert sorted(r.line() for r in found) == sorted("addr33\t%s\t%064x" % (orc.hex160(orc.hash160(*orc.point_of(keys[i] % orc.N), True)), keys[i]) for i in planted)
    assert ks.k_checked == n and ks.k_found == 3
    if name != "camp2":  # a device hash that disagrees with the engine's ends the call with the usual error, no key is reported
        FakeKdfDevice.corrupt = True
        ks = engine.KeySearch(engine.Filter(np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)), device_cls=FakeKdfDevice, kdf=name)
        with pytest.raises(engine.EclError, match="hash mismatch"):
            ks.cmd_mul_raw(lines[:5])
        assert ks.found == []
        FakeKdfDevice.corrupt = False
    with pytest.raises(ValueError):
        engine.KeySearch(flt, device_cls=FakeKdfDevice, kdf="md5")
