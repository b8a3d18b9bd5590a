"""`seed` on the GPU: ECL_KDF_BIP39 contexts - the flag and its refused neighbours, the self-test; the known answers through the ABI for
every address type; phrase lengths and alignments; passphrases; paths; malformed records; reuse; a call of more than one `mul` piece;
overflow and ecl_hip_fetch_found; a sparse real filter; KeySearch.cmd_seed; the host program.  The expected keys are tests/bip39_ref.py's
(hashlib + hmac; k G of a normal element from the oracle, pinned to the yardstick's own below); records are compared with those of
ecl_hip_mul_batch over these keys on a context without the flag.  All-ones filter unless stated.  Every GPU-using subprocess runs under
its own time limit."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import bip39_ref as R
import orc
from support import cli

pytestmark = pytest.mark.gpu
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
E_ARG, E_OVERFLOW = -1, -4
H = R.HARD
BIP44 = [44 | H, H, H, 0, 0]
TEN = [44 | H, 1, 2 | H, 0x7FFFFFFF, H, 5, 0xFFFFFFFF, 0, 7 | H, 1000000000]
A = R.PHRASE_A


def ser(k):
    x, y = orc.point_of(k)
    return bytes([2 | (y & 1)]) + x.to_bytes(32, "big")


def key_of(phrase, path, passphrase=b""):
    return R.key_of(phrase, path, passphrase, ser)


def key(a):
    return sorted(zip(a["key_offset"].tolist(), a["compressed"].tolist(), map(tuple, a["h160"].tolist())))


def test_the_oracles_public_keys_are_the_yardsticks_own():
    for k in (1, 2, 0xdc2a04, R.N - 1, 0xe284129cc0922579a535bbf4d1a3b25773090d28c909bc0fed73b5e0222cc372):
        assert ser(k) == R.ser_p(k)


@pytest.fixture(scope="module")
def pair():
    """a bip39 context and a plain one, both -a c with an all-ones filter"""
    from ecloop_amd import Device
    d, plain = Device(0, a33=True, bip39=True), Device(0, a33=True)
    d.set_bloom(ONES), plain.set_bloom(ONES)
    yield d, plain
    d.close(), plain.close()


@pytest.fixture(scope="module")
def phrases64():
    rnd = random.Random(39)
    words = ["abandon", "ability", "zoo", "wrong", "legal", "winner", "thank", "year", "wave", "sausage", "worth", "useful", "letter", "advice", "cage", "absurd"]
    return [" ".join(rnd.choice(words) for _ in range(rnd.choice((12, 15, 18, 21, 24)))).encode() for _ in range(64)]


def check(pair, phrases, path, passphrase=b"", reuse=False):
    """one seed_batch call: every phrase's record is that of the yardstick's key"""
    d, plain = pair
    want_k = [key_of(p, path, passphrase) for p in phrases]
    assert all(want_k)
    got, n = d.seed_batch(phrases, path, passphrase=passphrase, reuse=reuse, cap=len(phrases) + 8)
    ref, n2 = plain.mul_batch(want_k, cap=len(phrases) + 8)
    assert n == n2 == len(phrases) and key(got) == key(ref)
    return got


def test_the_flag_opens_beside_the_mul_contexts_and_its_refused_neighbours_stay_refused():
    from ecloop_amd import Device, capi
    lib = capi.load()
    A33, A65, P2SH, ENDO = capi.ADDR33, capi.ADDR65, capi.P2SH, capi.ENDO
    assert capi.BIP39 == 0x10000
    btc = [A33, A65, A33 | A65, P2SH, A33 | P2SH, A65 | P2SH, A33 | A65 | P2SH]
    for base in btc + [b | ENDO for b in btc] + [capi.ETH, capi.ETH | ENDO, capi.TR, capi.PUB, capi.PUB | ENDO]:
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, base | capi.BIP39, 0) == 0, base  # (the first open of a selection runs its self-test)
        if base in (A33 | A65, capi.ETH, capi.TR):
            assert lib.ecl_hip_selftest(h) == 0, base
        lib.ecl_hip_close(h)
        for kdf in (capi.KDF_KECCAK, capi.KDF_SHA3, capi.KDF_CAMP2):
            h = C.c_void_p()
            assert lib.ecl_hip_open(C.byref(h), 0, base | capi.BIP39 | kdf, 0) == E_ARG, (base, kdf)
    for base in (capi.PUB | capi.ORIGIN, capi.PUB | capi.INSERT, capi.PUB | capi.HERD, A33 | capi.PREFIX, capi.ETH | capi.PREFIX, capi.ETH | capi.MASK,
                 capi.ETH | capi.MASK | capi.ORIGIN, A33 | capi.PREFIX | capi.ORIGIN, 0, ENDO, capi.ETH | A33, capi.TR | ENDO, 8, 32):
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, base | capi.BIP39, 0) == E_ARG, base
    for kw in (dict(kdf="keccak"), dict(a33=False, pub=True, origin=True), dict(prefix=True), dict(a33=False, eth=True, mask=True)):
        with pytest.raises(ValueError):
            Device(0, bip39=True, **kw)


@pytest.mark.parametrize("ctx", ["c", "e", "s", "t", "x"])
def test_the_known_answers_through_the_abi(ctx):
    from ecloop_amd import Device
    kw = {"c": dict(a33=True), "e": dict(a33=False, eth=True), "s": dict(a33=False, p2sh=True), "t": dict(a33=False, tr=True), "x": dict(a33=False, pub=True)}[ctx]
    table = {"m": 0x1837c1be8e2995ec11cda2b066151be2cfb48adf9e47b151d46adab3a21cdf67,
             "m/44'/0'/0'/0/0": 0xe284129cc0922579a535bbf4d1a3b25773090d28c909bc0fed73b5e0222cc372,
             "m/84'/0'/0'/0/0": 0x4604b4b710fe91f584fff084e1a9159fe4f8408fff380596a604948474ce4fa3,
             "m/49'/0'/0'/0/0": 0x508c73a06f6b6c817238ba61be232f5080ea4616c54f94771156934666d38ee3,
             "m/44'/60'/0'/0/0": 0x1ab42cc412b618bdea3a599e3c9bae199ebf030895b039e9db1e30dafb12b727}
    d, plain = Device(0, bip39=True, **kw), Device(0, **kw)
    try:
        d.set_bloom(ONES), plain.set_bloom(ONES)
        for i, (path, k) in enumerate(table.items()):
            got, n = d.seed_batch([b"x", A], R.path_of(path), reuse=i > 0, cap=8)
            ref, _ = plain.mul_batch([key_of(b"x", R.path_of(path)), k], cap=8)
            assert n == 2 and key(got) == key(ref), path
        if ctx == "c":  # 1LqBGSKuX5yYUonjxT5qGfpUsXKYYWeabA is hash160 of 03aaeb52...af5e
            got, _ = d.seed_batch([A], BIP44, cap=8)
            x, y = orc.point_of(table["m/44'/0'/0'/0/0"])
            assert x == 0xaaeb52dd7494c361049de67cc680e83ebcbbbdbeb13637d92cd845f70308af5e and y & 1
            assert list(got[0]["h160"]) == orc.hash160(x, y, True)
        if ctx == "e":
            got, _ = d.seed_batch([A], R.path_of("m/44'/60'/0'/0/0"), cap=8)
            assert "".join("%08x" % int(w) for w in got[0]["h160"]) == "9858effd232b4033e47d90003d41ec34ecaeda94"
        got, n = d.seed_batch([A], [], passphrase=b"TREZOR", cap=8)  # another passphrase: another seed
        ref, _ = plain.mul_batch([0xcbedc75b0d6412c85c79bc13875112ef912fd1e756631b5a00330866f22ff184], cap=8)
        assert n == 1 and key(got) == key(ref)
    finally:
        d.close(), plain.close()


def test_300_phrases_of_1_to_260_bytes_at_mixed_alignments(pair):
    rnd = random.Random(512)
    lens = list(range(1, 261)) + [111, 112, 127, 128, 129, 215, 239, 240] + [rnd.randrange(1, 261) for _ in range(32)]
    phrases = [bytes(rnd.randrange(256) for _ in range(n)) for n in lens]
    assert len(phrases) == 300
    starts = np.cumsum([14] + [len(p) for p in phrases])[:-1]  # (behind the record: 8 + 4 + 2 bytes)
    assert {int(s) & 3 for s in starts} == {0, 1, 2, 3}
    check(pair, phrases, [7 | H], b"pw")


@pytest.mark.parametrize("n", [0, 1, 55, 99])
def test_passphrases_of_every_block_position(pair, phrases64, n):
    check(pair, phrases64[:8], [H], bytes(range(65, 65 + n)))


def raw_call(d, lines, cap=16):
    """ecl_hip_mul_batch_raw over the given lines, packed back to back -> (return code, records, count, last error)"""
    from ecloop_amd import capi
    text = b"".join(lines)
    table = np.zeros(len(lines), dtype=np.uint64)
    at = 0
    for i, l in enumerate(lines):
        table[i] = at | (len(l) << 32)
        at += len(l)
    buf = np.frombuffer(text, dtype=np.uint8)
    out = np.zeros(cap, dtype=capi.FOUND_DTYPE)
    cnt = C.c_uint32()
    rc = d.lib.ecl_hip_mul_batch_raw(d.h, buf.ctypes.data, len(text), table.ctypes.data, len(lines), out.ctypes.data, cap, C.byref(cnt))
    return rc, out[: min(cnt.value, cap)], cnt.value, d.lib.ecl_hip_last_error(d.h).decode()


def test_a_passphrase_of_100_bytes_and_a_path_of_11_elements_are_refused(pair):
    d, _ = pair
    rc, _, n, err = raw_call(d, [d.seed_record([], b"p" * 100), A])
    assert rc == E_ARG and n == 0 and "99" in err
    rc, _, n, err = raw_call(d, [d.seed_record([H] * 11), A])
    assert rc == E_ARG and n == 0 and "10" in err


@pytest.mark.parametrize("path", [[], [H], [0], BIP44, TEN, [0x7FFFFFFF], [0xFFFFFFFF], [0x80000000, 0x7FFFFFFF], [0xFFFFFFFF, 0]], ids=str)
def test_paths(pair, phrases64, path):
    check(pair, phrases64[:16], path)


def test_malformed_records_are_refused_and_nothing_is_launched(pair):
    from ecloop_amd import capi
    d, _ = pair
    good = d.seed_record(BIP44, b"pw")
    cov = d.coverage()
    for rec, word in ((good + b"\0", "length"), (good[:-1], "length"), (b"B38\0" + good[4:], "magic"), (b"", "shorter"), (A, "magic"),
                      (good[:4] + b"\x02" + good[5:], "reuse byte"), (good[:4] + b"\xff" + good[5:], "reuse byte"), (good[:7] + b"\x01" + good[8:], "reuse byte")):
        rc, _, n, err = raw_call(d, [rec, A])
        assert rc == E_ARG and n == 0 and word in err, (rec, err)
    assert d.coverage() == cov
    rc, recs, n, _ = raw_call(d, [good])  # the record alone
    assert rc == 0 and n == 0 and d.coverage() == cov
    # more than 2^22 phrases: the table's entries all name the one phrase
    text = np.frombuffer(good + A, dtype=np.uint8)
    m = (1 << 22) + 2
    table = np.full(m, len(good) | (len(A) << 32), dtype=np.uint64)
    table[0] = len(good) << 32
    out = np.zeros(8, dtype=capi.FOUND_DTYPE)
    cnt = C.c_uint32()
    assert d.lib.ecl_hip_mul_batch_raw(d.h, text.ctypes.data, len(text), table.ctypes.data, m, out.ctypes.data, 8, C.byref(cnt)) == E_ARG
    assert "2^22" in d.lib.ecl_hip_last_error(d.h).decode() and d.coverage() == cov
    check(pair, [A], BIP44)  # the context goes on


def test_reuse_gives_the_records_of_fresh_calls(pair, phrases64):
    d, _ = pair
    ph = phrases64[:24]
    fresh = {}
    for path in [BIP44[:4] + [i] for i in range(5)] + [[84 | H, H, H, 0, 0]]:
        got, n = d.seed_batch(ph, path, cap=64)
        assert n == len(ph)
        fresh[tuple(path)] = key(got)
    check(pair, ph, BIP44)
    for path, want in fresh.items():
        got, n = d.seed_batch(ph, list(path), reuse=True, cap=64)
        assert n == len(ph) and key(got) == want, path
    # reuse after a call on other phrases: those phrases' keys, whatever text the reuse call carries
    other = phrases64[24:48]
    check(pair, other, [H])
    want_k = [key_of(p, BIP44) for p in other]
    got, _ = d.seed_batch(ph, BIP44, reuse=True, cap=64)
    ref, _ = pair[1].mul_batch(want_k, cap=64)
    assert key(got) == key(ref)


def test_the_four_refusals_of_reuse(phrases64):
    from ecloop_amd import Device
    d = Device(0, a33=True, bip39=True)
    try:
        d.set_bloom(ONES)
        ph = phrases64[:4]
        rc, _, _, err = raw_call(d, [d.seed_record(BIP44, reuse=True)] + ph)
        assert rc == E_ARG and "no nodes" in err
        d.seed_batch(ph, BIP44, passphrase=b"pw", cap=8)
        rc, _, _, err = raw_call(d, [d.seed_record(BIP44, b"pw", reuse=True)] + ph[:3])
        assert rc == E_ARG and "number of phrases" in err
        d.seed_batch(ph, BIP44, passphrase=b"pw", cap=8)
        for other in (b"pW", b"p", b"pw2", b""):
            rc, _, _, err = raw_call(d, [d.seed_record(BIP44, other, reuse=True)] + ph)
            assert rc == E_ARG and "passphrase" in err, other
            d.seed_batch(ph, BIP44, passphrase=b"pw", cap=8)
        rc, _, _, _ = raw_call(d, [b"B38\0"] + ph)  # a call that did not succeed
        assert rc == E_ARG
        rc, _, _, err = raw_call(d, [d.seed_record(BIP44, b"pw", reuse=True)] + ph)
        assert rc == E_ARG and "did not succeed" in err
        d.seed_batch(ph, BIP44, passphrase=b"pw", cap=8)
        got, n = d.seed_batch(ph, BIP44, passphrase=b"pw", reuse=True, cap=2)  # an overflow is a success: the next reuse is served
        assert n == 4 and len(got) == 2
        got, n = d.seed_batch(ph, [H], passphrase=b"pw", reuse=True, cap=8)
        assert n == 4
    finally:
        d.close()


def test_a_call_of_more_than_one_mul_piece(pair, phrases64):
    """300 001 lines - the first `mul` piece holds 196 608, and the count is no multiple of 64 - of 64 distinct phrases; every record
    checked, coverage delta n - 1; then the same keys by reuse at another index"""
    import mul_ref
    from ecloop_amd import capi
    d, plain = pair
    np_ = 300_001
    assert len(mul_ref.pieces(np_)) >= 2
    rec = d.seed_record(BIP44)
    text = rec + b"".join(phrases64)
    starts = np.cumsum([len(rec)] + [len(p) for p in phrases64])[:-1].astype(np.uint64)
    one = starts | (np.array([len(p) for p in phrases64], dtype=np.uint64) << np.uint64(32))
    idx = np.arange(np_) % 64
    table = np.concatenate([[np.uint64(len(rec)) << np.uint64(32)], one[idx]]).astype(np.uint64)
    buf = np.frombuffer(text, dtype=np.uint8)
    out = np.zeros(np_ + 8, dtype=capi.FOUND_DTYPE)
    cnt = C.c_uint32()
    ref, _ = plain.mul_batch([key_of(p, BIP44) for p in phrases64], cap=64)
    want = np.zeros((64, 5), np.uint32)
    want[ref["key_offset"].astype(np.int64)] = ref["h160"]
    cov = d.coverage()
    assert d.lib.ecl_hip_mul_batch_raw(d.h, buf.ctypes.data, len(text), table.ctypes.data, np_ + 1, out.ctypes.data, np_ + 8, C.byref(cnt)) == 0
    assert cnt.value == np_ and tuple(b - a for a, b in zip(cov, d.coverage())) == (np_, np_, np_)
    got = out[:np_]
    assert np.array_equal(np.sort(got["key_offset"]), np.arange(np_)) and np.array_equal(got["h160"], want[got["key_offset"].astype(np.int64) % 64])
    # ... and a reuse = 1 call over the same pieces: the last index + 1 from the kept nodes, nothing of the text read but the record
    rec1 = d.seed_record(BIP44[:4] + [1], reuse=True)
    assert len(rec1) == len(rec)
    text1 = np.frombuffer(rec1 + b"\0" * (len(text) - len(rec1)), dtype=np.uint8)
    ref, _ = plain.mul_batch([key_of(p, BIP44[:4] + [1]) for p in phrases64], cap=64)
    want[ref["key_offset"].astype(np.int64)] = ref["h160"]
    cov = d.coverage()
    assert d.lib.ecl_hip_mul_batch_raw(d.h, text1.ctypes.data, len(text), table.ctypes.data, np_ + 1, out.ctypes.data, np_ + 8, C.byref(cnt)) == 0
    assert cnt.value == np_ and tuple(b - a for a, b in zip(cov, d.coverage())) == (np_, np_, np_)
    got = out[:np_]
    assert np.array_equal(np.sort(got["key_offset"]), np.arange(np_)) and np.array_equal(got["h160"], want[got["key_offset"].astype(np.int64) % 64])


def test_overflow_with_a_small_cap_then_fetch_found(pair, phrases64):
    d, plain = pair
    got, n = d.seed_batch(phrases64, [1 | H], cap=10)
    assert n == 64 and len(got) == 10
    rest = d.fetch_found(10, 54)
    ref, _ = plain.mul_batch([key_of(p, [1 | H]) for p in phrases64], cap=64)
    assert len(rest) == 54 and key(np.concatenate([got, rest])) == key(ref)


def test_a_sparse_real_filter_reports_the_planted_phrases_only(phrases64):
    from ecloop_amd import Device
    from ecloop_amd.engine import blf_add_host
    planted = [3, 17, 63]
    hs = np.array([orc.hash160(*orc.point_of(key_of(phrases64[i], BIP44)), True) for i in planted], dtype=np.uint32)
    words = np.zeros(4099, np.uint64)
    blf_add_host(words, hs)
    d = Device(0, a33=True, bip39=True)
    try:
        d.set_bloom(words)
        got, n = d.seed_batch(phrases64, BIP44, cap=64)
        assert n == 3 and sorted(got["key_offset"].tolist()) == planted
        assert key(got) == sorted((i, 1, tuple(int(v) for v in h)) for i, h in zip(planted, hs))
        got, n = d.seed_batch(phrases64, BIP44[:4] + [1], reuse=True, cap=64)
        assert n == 0
    finally:
        d.close()


def test_keysearch_cmd_seed_finds_and_verifies_the_planted_keys(phrases64, tmp_path):
    from ecloop_amd.engine import KeySearch, load_filter
    plan = [(5, "m/44'/0'/0'/0/0"), (9, "m/44'/0'/0'/0/3"), (40, "m/84'/0'/0'/0/1")]
    keys = [key_of(phrases64[i], R.path_of(p), b"pw") for i, p in plan]
    lst = tmp_path / "list.txt"
    lst.write_text("".join(orc.hex160(orc.hash160(*orc.point_of(k), True)) + "\n" for k in keys))
    ks = KeySearch(load_filter(str(lst)), device=0, bip39=True)
    try:
        found = ks.cmd_seed(phrases64, ["m/44'/0'/0'/0/0", "m/84'/0'/0'/0/0"], count=4, passphrase=b"pw")
        assert sorted((r.pk, r.path, r.phrase) for r in found) == sorted((k, p, phrases64[i]) for k, (i, p) in zip(keys, plan))
        assert ks.k_checked == 64 * 8 and all(r.line().endswith("\t%s\t%s" % (r.path, r.phrase.decode())) for r in found)
    finally:
        ks.close()
    with pytest.raises(ValueError):
        KeySearch(load_filter(str(lst)), device=0, bip39=True, kdf="keccak")
    KeySearch(load_filter(str(lst)), device=0, bip39=True, kdf="sha256").close()  # "sha256" is no kdf, here as everywhere


def seed_case(tmp_path, phrases64):
    """50 phrases, two paths, five indexes each, a passphrase; four planted (phrase, path) pairs -> (arguments, phrase file, the found lines)"""
    phrases = phrases64[:50]
    plan = [(0, "m/44'/0'/0'/0/0"), (17, "m/44'/0'/0'/0/4"), (33, "m/84'/0'/0'/1/2"), (49, "m/84'/0'/0'/1/0")]
    want, hs = [], []
    for i, p in plan:
        k = key_of(phrases[i], R.path_of(p), b"pw")
        h = orc.hex160(orc.hash160(*orc.point_of(k), True))
        hs.append(h)
        want.append("addr33: %s <- %064x %s %s" % (h, k, p, phrases[i].decode()))
    lst = tmp_path / "list.txt"
    lst.write_text("".join(h + "\n" for h in hs))
    ph = tmp_path / "phrases.txt"
    ph.write_bytes(b"\n".join(phrases) + b"\n")
    return ["seed", "-f", str(lst), "-path", "m/44'/0'/0'/0/0", "-path", "m/84h/0h/0h/1/0", "-n", "5", "-pass", "pw"], str(ph), sorted(want)


def test_cli_seed_finds_exactly_the_yardsticks_lines(cli, tmp_path, phrases64):
    args, ph, want = seed_case(tmp_path, phrases64)
    out = tmp_path / "found.txt"
    pr = subprocess.run([cli] + args + ["-o", str(out)], stdin=open(ph, "rb"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-2000:]
    assert sorted(l for l in pr.stdout.decode().splitlines() if " <- " in l) == want
    rows = sorted(out.read_text().splitlines())
    assert rows == sorted("\t".join(w.replace(":", "", 1).replace(" <- ", " ").split(" ", 4)) for w in want)  # tab-separated, the phrase last
    assert b"4 / 500" in pr.stderr  # 50 phrases x 2 paths x 5 indexes


def test_cli_seed_stops_on_a_key_the_device_does_not_confirm(cli, tmp_path, phrases64):
    """ECLOOP_HIP_TEST_SEED_DISAGREE flips the lowest bit of the host's key of every hit: what a device derivation that disagrees with the
    host's looks like - the run ends with the hash mismatch error and prints no key"""
    args, ph, _ = seed_case(tmp_path, phrases64)
    env = dict(os.environ, ECLOOP_HIP_TEST_SEED_DISAGREE="1")
    pr = subprocess.run([cli] + args, stdin=open(ph, "rb"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert pr.returncode != 0 and b"hash mismatch" in pr.stderr, pr.stderr[-2000:]
    assert b" <- " not in pr.stdout, pr.stdout
