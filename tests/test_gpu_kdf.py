"""`mul -raw -kdf` on the GPU: the flags of ecl_hip_open and the self-test with the known answers; every line length and start alignment
for Keccak-256 and SHA3-256 against ecl_hip_mul_batch over the digests of tests/kdf_ref.py; the 2031-fold form against the host program's
independent C; every address type; a call of several pieces with the table in and out of the text's order; the calls the bits must not
touch; a line outside the text; and the host program end to end.  All-ones filter unless stated.  Every GPU-using subprocess runs under
its own time limit."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import kdf_ref
import mul_ref
import orc
from support import cli
from walk_ref import canon, difference

pytestmark = pytest.mark.gpu
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
LENGTHS = list(range(0, 301)) + [407, 408, 409, 1000, 4000]
E_ARG, E_SELFTEST = -1, -7


def limbs_of_digests(digests):
    """32-byte digests -> (n, 4) uint64 little-endian limbs of the big-endian numbers"""
    a = np.frombuffer(b"".join(digests), dtype=">u8").reshape(-1, 4)
    return np.ascontiguousarray(a[:, ::-1]).astype(np.uint64)


def key(a):
    return sorted(zip(a["key_offset"].tolist(), a["compressed"].tolist(), map(tuple, a["h160"].tolist())))


def test_every_valid_combination_opens_and_passes_its_selftest_and_the_five_companions_are_refused():
    from ecloop_amd import capi
    lib = capi.load()
    A33, A65, P2SH, ENDO = capi.ADDR33, capi.ADDR65, capi.P2SH, capi.ENDO
    btc = [A33, A65, A33 | A65, P2SH, A33 | P2SH, A65 | P2SH, A33 | A65 | P2SH]
    bases = btc + [b | ENDO for b in btc] + [capi.ETH, capi.ETH | ENDO, capi.TR, capi.PUB, capi.PUB | ENDO]
    assert len(bases) == 19
    for base in bases:
        for kdf in (capi.KDF_KECCAK, capi.KDF_SHA3, capi.KDF_CAMP2):
            h = C.c_void_p()
            assert lib.ecl_hip_open(C.byref(h), 0, base | kdf, 0) == 0, (base, kdf)  # (the first open of a selection runs its self-test)
            if base in (A33 | A65, capi.ETH, capi.TR, capi.PUB | ENDO):  # ... and asked for: the base context's, then the hash's known answers
                assert lib.ecl_hip_selftest(h) == 0, (base, kdf)
            lib.ecl_hip_close(h)
    refused = [capi.PUB | capi.ORIGIN, capi.PUB | capi.INSERT, capi.PUB | capi.HERD, A33 | capi.PREFIX, capi.ETH | capi.PREFIX, capi.ETH | capi.MASK,
               capi.ETH | capi.MASK | capi.ORIGIN, A33 | capi.PREFIX | capi.ORIGIN]
    for base in refused:
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, base, 0) == 0, base  # valid without the bits ...
        lib.ecl_hip_close(h)
        for kdf in (capi.KDF_KECCAK, capi.KDF_SHA3, capi.KDF_CAMP2):
            h = C.c_void_p()
            assert lib.ecl_hip_open(C.byref(h), 0, base | kdf, 0) == E_ARG, (base, kdf)  # ... and ECL_E_ARG with them
    for kdf in (capi.KDF_KECCAK, capi.KDF_SHA3, capi.KDF_CAMP2):  # the bits are no type: alone, or beside a refused set, they open nothing
        for base in (0, ENDO, capi.ETH | A33, capi.TR | ENDO, 8, 32):
            h = C.c_void_p()
            assert lib.ecl_hip_open(C.byref(h), 0, base | kdf, 0) == E_ARG, (base, kdf)


@pytest.mark.parametrize("name", ["keccak", "sha3"])
def test_every_length_and_alignment_gives_the_records_of_the_reference_digests(name):
    """the comparison test_mul_batch_raw_hashes_lines_on_the_device makes for SHA-256: one raw call over lines of every length 0..300 and
    407, 408, 409, 1000, 4000, packed back to back (capi.Device.mul_batch_raw), against mul_batch on a context without the bits"""
    from ecloop_amd import Device
    rnd = random.Random(1600)
    lines = [bytes(rnd.randrange(256) for _ in range(n)) for n in LENGTHS]
    starts = np.concatenate([[0], np.cumsum([len(l) for l in lines])[:-1]])
    assert {int(s) & 3 for s in starts} == {0, 1, 2, 3}  # all four start alignments occur
    want_k = [kdf_ref.scalar(name, l) for l in lines]
    d, plain = Device(0, a33=True, a65=True, kdf=name), Device(0, a33=True, a65=True)
    try:
        d.set_bloom(ONES), plain.set_bloom(ONES)
        got, n1 = d.mul_batch_raw(lines, cap=2 * len(lines))
        ref, n2 = plain.mul_batch(want_k, cap=2 * len(lines))
        assert n1 == n2 == 2 * len(lines)
        assert key(got) == key(ref)
        # "" and "abc": the known digests, as literals, through the oracle's hash160
        g, _ = d.mul_batch_raw([b"", b"abc"], cap=8)
        assert len(g) == 4
        known = {"keccak": ("c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470", "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"),
                 "sha3": ("a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a", "3a985da74fe225b2045c172d6bd390bd855f086e3e9d525b46bfe24511431532")}[name]
        for rec in g:
            k = int(known[int(rec["key_offset"])], 16) % orc.N
            assert list(rec["h160"]) == orc.hash160(*orc.point_of(k), bool(rec["compressed"]))
    finally:
        d.close(), plain.close()


def test_camp2_against_the_host_programs_digests_and_the_known_answers(cli):
    """300 lines of 0..140 bytes; the expected digests are the host program's (`parse -raw -kdf camp2`: independent C on 64-bit lanes,
    pinned to tests/kdf_ref.py by the known answers in tests/test_kdf_host.py).  The reader lists non-empty lines only, so the empty
    line's digest is the known answer itself."""
    from ecloop_amd import Device
    rnd = random.Random(2031)
    alphabet = b"abcdefghijklmnopqrstuvwxyz0123456789 !"
    lens = list(range(0, 141)) + [rnd.randrange(1, 141) for _ in range(156)]
    lines = [b"", b"abc", b"password"] + [bytes(rnd.choice(alphabet) for _ in range(n)) for n in lens]
    assert len(lines) == 300
    known = ["26d412aa8b9fea49149a7dbf8b19672d8813f741842ac1847571d335908cbe65", "7a44789ed3cd85861c0bbf9693c7e1de1862dd4396c390147ecf1275099c6e6f",
             "5e225b381fcf02bd5577885f19b9472234c117dc44df6b59aca6690471dea0a0"]
    live = [l for l in lines if l]
    pr = subprocess.run([cli, "parse", "-raw", "-kdf", "camp2"], input=b"\n".join(live) + b"\n", capture_output=True, timeout=120)
    assert pr.returncode == 0, pr.stderr
    host = dict(zip(live, pr.stdout.decode().split()))
    assert len(host) == len(set(live)) and host[b"abc"] == known[1] and host[b"password"] == known[2]
    want_k = [int(known[0] if not l else host[l], 16) for l in lines]
    d, plain = Device(0, a33=True, a65=True, kdf="camp2"), Device(0, a33=True, a65=True)
    try:
        d.set_bloom(ONES), plain.set_bloom(ONES)
        got, n1 = d.mul_batch_raw(lines, cap=2 * len(lines))
        ref, n2 = plain.mul_batch(want_k, cap=2 * len(lines))
        assert n1 == n2 == 2 * len(lines) and key(got) == key(ref)
        for rec in got[got["key_offset"] < 3]:
            k = int(known[int(rec["key_offset"])], 16) % orc.N
            assert list(rec["h160"]) == orc.hash160(*orc.point_of(k), bool(rec["compressed"]))
    finally:
        d.close(), plain.close()


@pytest.fixture(scope="module")
def phrases200():
    rnd = random.Random(200)
    lines = [bytes(rnd.randrange(32, 127) for _ in range(rnd.randrange(1, 150))) for _ in range(200)]
    return lines, mul_ref.MulRef(limbs_of_digests([kdf_ref.digest("keccak", l) for l in lines]))


@pytest.mark.parametrize("ctx", ["e", "t", "x", "s", "cu -endo"])
def test_every_address_type_reports_the_reference_records_of_the_keccak_digests(phrases200, ctx):
    """200 phrases with kdf="keccak" on the contexts of -a e, -a t, -a x, -a s and -a cu -endo (`mul` has no endomorphism images: endo 0);
    every record against tests/mul_ref.py's tables - eth_ref, tr_ref, the oracle's points and hash160, p2sh_ref - for the digests"""
    from ecloop_amd import Device
    lines, ref = phrases200
    name = ctx.split()[0]
    kw = dict(mul_ref.CONTEXTS[name][1], endo=ctx.endswith("-endo"))
    want = ref.records(name)
    assert len(want) == len(name) * 200
    d = Device(0, kdf="keccak", **kw)
    try:
        d.set_bloom(ONES)
        got, n = d.mul_batch_raw(lines, cap=len(want) + 16)
        assert n == len(got) == len(want) and difference(canon(got), want) == ""
    finally:
        d.close()


def test_a_call_of_three_pieces_with_the_table_in_text_order_and_reversed():
    """the SHA-256 test's shape (lines of 1..40 bytes, test_mul_batch_raw_in_pieces_table_in_any_order_against_the_oracle) at a length that
    mul_pieces cuts into three (mul_ref.pieces; 700 001 lines are two): the text travels with the pieces, a reversed table raises the
    kernel's flag [1] and the call is run again with the whole text first - the coverage deltas of the SHA-256 test; every line's two
    hashes against the oracle's for the digests of kdf_ref's numpy form"""
    from ecloop_amd import Device, capi
    rng = np.random.default_rng(1600)
    n = 800_001
    assert len(mul_ref.pieces(n)) >= 3
    ln = rng.integers(1, 41, n).astype(np.uint64)
    starts = np.concatenate([[0], np.cumsum(ln + 1)[:-1]]).astype(np.uint64)
    tot = int(ln.sum()) + n
    text = rng.integers(32, 127, tot, dtype=np.uint8)
    text[(starts + ln).astype(np.int64)] = 10
    dg = kdf_ref.digests_many("keccak", text, starts, ln)
    for i in (0, 1, n // 2, n - 1):  # the numpy form against the pure one
        assert bytes(dg[i]) == kdf_ref.digest("keccak", text[int(starts[i]): int(starts[i] + ln[i])].tobytes())
    ks = np.ascontiguousarray(np.ascontiguousarray(dg).view(">u8").reshape(n, 4)[:, ::-1]).astype(np.uint64)
    h33, h65, ok = orc.mul_hash160_many(ks, a33=True, a65=True)
    assert ok.all()
    in_order = starts | (ln << np.uint64(32))
    d = Device(0, a33=True, a65=True, kdf="keccak")
    try:
        d.set_bloom(ONES)
        out = np.zeros(2 * n, dtype=capi.FOUND_DTYPE)
        cnt = C.c_uint32()
        for name, perm in (("text order", np.arange(n)), ("reversed", np.arange(n)[::-1].copy())):
            table = np.ascontiguousarray(in_order[perm])
            cov = d.coverage()
            assert d.lib.ecl_hip_mul_batch_raw(d.h, text.ctypes.data, tot, table.ctypes.data, n, out.ctypes.data, 2 * n, C.byref(cnt)) == 0, name
            assert cnt.value == 2 * n, name
            assert tuple(b - a for a, b in zip(cov, d.coverage())) == (n, n, n if name == "text order" else 2 * n), name
            got = out[: 2 * n]
            line = perm[got["key_offset"].astype(np.int64)]
            comp = got["compressed"].astype(bool)
            assert np.array_equal(got["h160"][comp], h33[line[comp]]) and np.array_equal(got["h160"][~comp], h65[line[~comp]]), name
            assert comp.sum() == n and len(set(line[comp].tolist())) == n, name
    finally:
        d.close()


@pytest.mark.parametrize("name", ["keccak", "sha3", "camp2"])
def test_add_range_and_mul_batch_are_those_of_the_context_without_the_bits(name):
    from ecloop_amd import Device
    rnd = random.Random(77)
    ks = [rnd.getrandbits(256) for _ in range(997)] + [0, orc.N, orc.N + 5]
    d, plain = Device(0, a33=True, a65=True, kdf=name), Device(0, a33=True, a65=True)
    try:
        d.set_bloom(ONES), plain.set_bloom(ONES)
        a, na = d.add_range(0x123456789, 1 << 16, cap=1 << 17)
        b, nb = plain.add_range(0x123456789, 1 << 16, cap=1 << 17)
        assert na == nb == 1 << 17 and difference(canon(a), canon(b)) == ""
        a, na = d.mul_batch(ks, cap=2000)
        b, nb = plain.mul_batch(ks, cap=2000)
        assert na == nb == 2 * 998 and difference(canon(a), canon(b)) == ""
    finally:
        d.close(), plain.close()


@pytest.mark.parametrize("name", ["keccak", "sha3", "camp2"])
def test_a_line_outside_the_text_is_refused(name):
    from ecloop_amd import Device, capi
    d = Device(0, a33=True, a65=True, kdf=name)
    try:
        d.set_bloom(ONES)
        text = np.frombuffer(b"0123456789", dtype=np.uint8)
        table = np.array([0 | (4 << 32), 8 | (3 << 32)], dtype=np.uint64)  # the second line ends one byte after the text
        out = np.zeros(8, dtype=capi.FOUND_DTYPE)
        cnt = C.c_uint32()
        assert d.lib.ecl_hip_mul_batch_raw(d.h, text.ctypes.data, 10, table.ctypes.data, 2, out.ctypes.data, 8, C.byref(cnt)) == E_ARG
        assert b"outside the text" in d.lib.ecl_hip_last_error(d.h)
        got, n = d.mul_batch_raw([b"0123", b"89"], cap=8)  # the context goes on
        assert n == 4 and {int(r["key_offset"]) for r in got} == {0, 1}
    finally:
        d.close()


def run_mul(cli, args, stdin_path):
    pr = subprocess.run([cli, "mul"] + args, stdin=open(stdin_path, "rb"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-2000:]
    out = pr.stdout.decode(errors="replace")
    return sorted(l for l in out.splitlines() if ": " in l and " <- " in l), out


def test_cli_mul_raw_kdf_prints_the_planted_eth_lines_with_the_digest_as_key(cli, tmp_path):
    import eth_ref
    eth_of = lambda k: eth_ref.eth_hex(*orc.point_of(k % orc.N))
    others = [b"phrase %d" % i for i in range(5000)]
    planted = [b"eth test phrase", b"correct horse battery staple", b"keccak not sha3"]
    want = ["eth: %s <- %064x" % (eth_of(k), k) for k in (kdf_ref.scalar("keccak", p) for p in planted)]
    lst = tmp_path / "planted.txt"
    lst.write_text("".join("0x" + l.split()[1] + "\n" for l in want))
    ph = tmp_path / "phrases.txt"
    ph.write_bytes(b"\n".join(others[:1000] + planted[:1] + others[1000:4000] + planted[1:] + others[4000:4997]) + b"\n")
    found, out = run_mul(cli, ["-raw", "-kdf", "keccak", "-a", "e", "-f", str(lst)], str(ph))
    assert found == sorted(want) and "~ eth: 1 |" in out, out
    found, out = run_mul(cli, ["-raw", "-a", "e", "-f", str(lst)], str(ph))  # the same phrases under SHA-256 are other keys
    assert found == [], out
    one = b"ethercamp brain wallet"
    k = int(subprocess.run([cli, "parse", "-raw", "-kdf", "camp2"], input=one + b"\n", capture_output=True, timeout=60, check=True).stdout.split()[0], 16)
    assert int("5e225b381fcf02bd5577885f19b9472234c117dc44df6b59aca6690471dea0a0", 16) == int(
        subprocess.run([cli, "parse", "-raw", "-kdf", "camp2"], input=b"password\n", capture_output=True, timeout=60, check=True).stdout.split()[0], 16)
    lst2 = tmp_path / "camp2.txt"
    lst2.write_text("0x%s\n" % eth_of(k))
    ph2 = tmp_path / "phrases2.txt"
    ph2.write_bytes(b"\n".join(others[:321] + [one] + others[321:499]) + b"\n")
    found, out = run_mul(cli, ["-raw", "-kdf", "camp2", "-a", "e", "-f", str(lst2)], str(ph2))
    assert found == ["eth: %s <- %064x" % (eth_of(k), k)], out


@pytest.mark.parametrize("letters", ["c", "u", "cs"])
def test_cli_rederives_bitcoin_type_hits_under_kdf_and_stops_on_a_disagreement(cli, tmp_path, letters):
    """plain `mul -raw` prints Bitcoin-type hits unverified, as the reference does; under -kdf every hit is re-derived on the device from the
    host's digest.  The planted phrase is found with key = digest; with the host's digest made to disagree (the test hook
    ECLOOP_HIP_TEST_KDF_DISAGREE flips its lowest bit: what a wrong device hash looks like from the host) the run ends with the hash
    mismatch error and prints no key; plain -raw ignores the hook"""
    import hashlib
    import p2sh_ref
    others = [b"phrase %d" % i for i in range(300)]
    one = b"keccak brain wallet"
    label = {"c": "addr33", "u": "addr65", "cs": "p2sh"}[letters]
    def h160_of(k):
        x, y = orc.point_of(k % orc.N)
        h33 = orc.hash160(x, y, True)
        return orc.hash160(x, y, False) if letters == "u" else [int(v) for v in p2sh_ref.p2sh_of_h33(h33)] if letters == "cs" else h33
    k = kdf_ref.scalar("keccak", one)
    ksha = int.from_bytes(hashlib.sha256(one).digest(), "big")
    lst = tmp_path / "list.txt"
    lst.write_text(orc.hex160(h160_of(k)) + "\n" + orc.hex160(h160_of(ksha)) + "\n")
    ph = tmp_path / "phrases.txt"
    ph.write_bytes(b"\n".join(others[:123] + [one] + others[123:]) + b"\n")
    args = ["-raw", "-kdf", "keccak", "-a", letters, "-f", str(lst)]
    found, out = run_mul(cli, args, str(ph))
    assert found == ["%s: %s <- %064x" % (label, orc.hex160(h160_of(k)), k)], out
    env = dict(os.environ, ECLOOP_HIP_TEST_KDF_DISAGREE="1")
    pr = subprocess.run([cli, "mul"] + args, stdin=open(str(ph), "rb"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert pr.returncode != 0 and b"hash mismatch" in pr.stderr, pr.stderr[-2000:]
    assert b" <- " not in pr.stdout, pr.stdout
    pr = subprocess.run([cli, "mul", "-raw", "-a", letters, "-f", str(lst)], stdin=open(str(ph), "rb"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                        timeout=300, env=env)
    assert pr.returncode == 0 and ("%s: %s <- %064x" % (label, orc.hex160(h160_of(ksha)), ksha)).encode() in pr.stdout, pr.stderr[-2000:]
