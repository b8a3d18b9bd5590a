"""`seed` without a GPU: the yardstick (tests/bip39_ref.py) pinned to the published BIP39 / BIP32 answers; the device headers sha512.h /
bip39.h compiled for the host (csrc/tools/bip39_host.cpp) against it - SHA-512 at every length to 300 bytes and at support.SEED_LONG_LENS (4 to 32 blocks), HMAC keys of the same lengths, PBKDF2 iterations and
passphrases, the gather at every alignment, CKDpriv, the node validity rules - and as a program under the sanitizers; the host program's
own derivation through `seed -keys`, and every refusal of the command; the binding's constant, the header, the record seed_batch builds;
engine.bip39_key and parse_path; the static figures of the two kernels."""
import ctypes as C
import hashlib
import hmac
import os
import random
import re
import subprocess

import numpy as np
import pytest

import bip39_ref as R
from support import ROOT, SEED_LONG_LENS, cli, host_lib, host_program, run_program

H = R.HARD
A = R.PHRASE_A
TABLE = {"m": "1837c1be8e2995ec11cda2b066151be2cfb48adf9e47b151d46adab3a21cdf67",
         "m/44'/0'/0'/0/0": "e284129cc0922579a535bbf4d1a3b25773090d28c909bc0fed73b5e0222cc372",
         "m/84'/0'/0'/0/0": "4604b4b710fe91f584fff084e1a9159fe4f8408fff380596a604948474ce4fa3",
         "m/49'/0'/0'/0/0": "508c73a06f6b6c817238ba61be232f5080ea4616c54f94771156934666d38ee3",
         "m/44'/60'/0'/0/0": "1ab42cc412b618bdea3a599e3c9bae199ebf030895b039e9db1e30dafb12b727"}


def test_the_yardstick_gives_the_published_answers():
    s = R.seed_of(A).hex()
    assert s.startswith("5eb00bbddcf06908") and s.endswith("ce9e38e4")
    s = R.seed_of(A, b"TREZOR").hex()
    assert s.startswith("c55257c360c07c72") and s.endswith("e7463b04")
    for path, k in TABLE.items():
        assert "%064x" % R.key_of(A, R.path_of(path)) == k, path
    assert R.ser_p(int(TABLE["m/44'/0'/0'/0/0"], 16)).hex() == "03aaeb52dd7494c361049de67cc680e83ebcbbbdbeb13637d92cd845f70308af5e"
    assert "%064x" % R.key_of_seed(bytes(range(16)), R.path_of("m/0'/1/2'/2/1000000000")) == "471b76e389e528d6de6d816857e012c5455051cad6660850e58372a6c3e6e7c8"
    long = b" ".join([b"abstract"] * 24)
    assert len(long) == 215 and R.seed_of(long).hex().startswith("377417f3d21974307929527f25246cef")


@pytest.fixture(scope="module")
def K(tmp_path_factory):
    lib = host_lib(tmp_path_factory, "bip39_host.cpp")
    V = C.c_void_p
    lib.bh_sha512.argtypes = [V, V, C.c_uint32, V]
    lib.bh_hmac.argtypes = [V, C.c_uint64, C.c_char_p, C.c_uint32, V]
    lib.bh_seed.argtypes = [V, V, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, V]
    lib.bh_master.argtypes = [V, C.c_uint32, V, C.c_uint32, C.c_char_p, C.c_uint32, V]
    lib.bh_ckd.argtypes = [V, V, C.c_uint32, V, C.c_uint32]
    lib.bh_master_rule.argtypes = [V, V]
    lib.bh_child_rule.argtypes = [V, V, V]
    return lib


def packed(lines, lead=0):
    """lines back to back behind `lead` bytes -> (the text in a buffer of the library's size: the bytes, rounded up to words, and two
    spare words; the table; the text's length).  The last line ends on the text's last byte."""
    table, at = [], lead
    for l in lines:
        table.append(at | (len(l) << 32))
        at += len(l)
    blob = b"\xA5" * lead + b"".join(lines)
    text = np.zeros(((len(blob) + 3) // 4 + 2) * 4, np.uint8)
    text[: len(blob)] = np.frombuffer(blob, np.uint8)
    return text, np.array(table, dtype=np.uint64), len(blob)


def words_bytes(a):
    """rows of big-endian 64-bit words -> bytes"""
    return [b"".join(int(w).to_bytes(8, "big") for w in row) for row in a]


def k_int(words):
    return sum(int(w) << (32 * i) for i, w in enumerate(words))


def test_sha512_at_every_length_and_alignment(K):
    """every length 0 ... 300, then support.SEED_LONG_LENS: 4 to 32 blocks - sha512_text's block loop past its third pass and the gather of
    sha512_text_word at positions past 384, which nothing read before - with the 111 / 112 mod 128 padding spill at every block up to the 8th"""
    rnd = random.Random(512)
    lens = list(range(0, 301)) + SEED_LONG_LENS
    assert {111, 112, 127, 128, 129, 239, 240, 495, 496, 1007, 1008, 1024, 4000} <= set(lens)
    lines = [bytes(rnd.randrange(256) for _ in range(n)) for n in lens]
    want = [hashlib.sha512(l).digest() for l in lines]
    seen = set()
    for lead in range(4):
        text, table, _ = packed(lines, lead)
        seen |= {int(t) & 3 for t in table}
        out = np.zeros((len(lines), 8), np.uint64)
        K.bh_sha512(text.ctypes.data, table.ctypes.data, len(lines), out.ctypes.data)
        assert words_bytes(out) == want, lead
    assert seen == {0, 1, 2, 3}


def test_hmac_with_keys_around_the_block_size(K):
    """... and keys of support.SEED_LONG_LENS bytes: bip39_key_block's hashed branch over 4 to 32 blocks"""
    rnd = random.Random(128)
    for klen in [0, 1, 127, 128, 129, 215, 300] + SEED_LONG_LENS:
        key = bytes(rnd.randrange(256) for _ in range(klen))
        for lead in range(4):
            text, table, _ = packed([key], lead)
            for mlen in (0, 1, 37, 64, 111):
                msg = bytes(rnd.randrange(256) for _ in range(mlen))
                out = np.zeros(8, np.uint64)
                assert K.bh_hmac(text.ctypes.data, int(table[0]), msg, mlen, out.ctypes.data) == 0
                assert words_bytes([out])[0] == hmac.new(key, msg, hashlib.sha512).digest(), (klen, lead, mlen)


def test_pbkdf2_iterations_passphrases_and_the_gather(K):
    rnd = random.Random(2048)
    phrases = [A, b"x", bytes(rnd.randrange(256) for _ in range(128)), bytes(rnd.randrange(256) for _ in range(129)), b" ".join([b"abstract"] * 24)]
    for rounds in (1, 2, 3, 2048):
        for plen in (0, 1, 55, 99):
            pw = bytes(rnd.randrange(1, 256) for _ in range(plen))
            for lead in (range(4) if rounds < 2048 else (3,)):  # start alignments 0 ... 3, the text ending with the last phrase
                text, table, _ = packed(phrases, lead)
                out = np.zeros((len(phrases), 8), np.uint64)
                K.bh_seed(text.ctypes.data, table.ctypes.data, len(phrases), pw, plen, rounds, out.ctypes.data)
                assert words_bytes(out) == [hashlib.pbkdf2_hmac("sha512", p, b"mnemonic" + pw, rounds, 64) for p in phrases], (rounds, plen, lead)


def test_the_master_stage_writes_the_yardsticks_nodes(K):
    phrases = [A, b"zoo " * 11 + b"wrong", b"q"]
    for pw in (b"", b"TREZOR"):
        text, table, nbytes = packed(phrases, 1)
        nodes = np.zeros((len(phrases), 16), np.uint32)
        K.bh_master(text.ctypes.data, nbytes, table.ctypes.data, len(phrases), pw, len(pw), nodes.ctypes.data)
        for p, node in zip(phrases, nodes):
            k, c = R.master_of(R.seed_of(p, pw))
            assert k_int(node[:8]) == k and b"".join(int(w).to_bytes(4, "big") for w in node[8:]) == c
    assert "%064x" % k_int(nodes[0][:8]) == "cbedc75b0d6412c85c79bc13875112ef912fd1e756631b5a00330866f22ff184"
    # a line outside the text is read as empty, and nothing behind the text is touched
    bad = np.array([int(table[-1]) + (5 << 32)], dtype=np.uint64)
    K.bh_master(text.ctypes.data, nbytes, bad.ctypes.data, 1, b"", 0, nodes.ctypes.data)
    assert k_int(nodes[0][:8]) == R.master_of(R.seed_of(b""))[0]


def ckd(K, k, c, index, pub=None):
    kw = np.array([(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint32)
    cw = np.frombuffer(c, dtype=">u4").astype(np.uint32)
    x = int.from_bytes(pub[1:], "big") if pub else 0
    px = np.array([(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint32)
    ok = K.bh_ckd(kw.ctypes.data, cw.ctypes.data, index, px.ctypes.data, pub[0] & 1 if pub else 0)
    return (k_int(kw), b"".join(int(w).to_bytes(4, "big") for w in cw)) if ok else None


def test_ckdpriv_hardened_and_normal_at_the_extreme_indexes(K):
    k, c = R.master_of(R.seed_of(A))
    pub = R.ser_p(k)
    for index in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        assert ckd(K, k, c, index, None if index & H else pub) == R.ckd(k, c, index), index
    # BIP32's test vector 1 down m/0'/1/2'/2/1000000000
    k, c = R.master_of(bytes(range(16)))
    for index in R.path_of("m/0'/1/2'/2/1000000000"):
        k, c = ckd(K, k, c, index, None if index & H else R.ser_p(k))
    assert "%064x" % k == "471b76e389e528d6de6d816857e012c5455051cad6660850e58372a6c3e6e7c8"


def test_the_node_validity_rules_on_planted_values(K):
    def I_of(il, ir=b"\x11" * 32):
        return np.frombuffer(il.to_bytes(32, "big") + ir, dtype=">u8").astype(np.uint64)

    def master(il):
        node = np.zeros(16, np.uint32)
        K.bh_master_rule(I_of(il).ctypes.data, node.ctypes.data)
        return k_int(node[:8])

    def child(il, k):
        kw = np.array([(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint32)
        cw = np.zeros(8, np.uint32)
        ok = K.bh_child_rule(kw.ctypes.data, cw.ctypes.data, I_of(il).ctypes.data)
        assert (k_int(kw) == k and not cw.any()) if not ok else bytes(cw.astype(">u4").tobytes()) == b"\x11" * 32
        return k_int(kw) if ok else None

    N = R.N
    assert [master(v) for v in (0, 1, N - 1, N, N + 1, 2**256 - 1)] == [0, 1, N - 1, 0, 0, 0]
    assert child(0, 5) == 5 and child(N - 1, 5) == 4 and child(N, 5) is None and child(2**256 - 1, 5) is None
    assert child(N - 5, 5) is None and child(1, N - 1) is None  # I_L + k = 0 mod n
    assert child(N - 1, N - 1) == N - 2  # the sum passes 2^256: the carry
    assert child(N - 1, 1) is None and child(N - 1, 2) == 1
    rnd = random.Random(32)
    for _ in range(200):
        il, k = rnd.randrange(2**256), rnd.randrange(1, N)
        want = R.child_of(il.to_bytes(32, "big") + b"\x11" * 32, k)
        assert child(il, k) == (want[0] if want else None)


def test_the_harness_as_a_program_under_the_sanitizers(tmp_path):
    """bip39_host.cpp's own main, built with ASan + UBSan and run directly: the known answers; every length 0 ... 1100, then 2000 and 4000, as the last line of a
    heap block that ends with the text's two spare words, at the four alignments (a gather that read behind them is a heap overflow; a
    shift by 32 in the masks is undefined behaviour); the validity rules"""
    pr = run_program(host_program(tmp_path, "bip39_host.cpp", ["-O1"]), timeout=300)
    assert pr.returncode == 0 and pr.stdout.strip() == "ok", (pr.stdout, pr.stderr[-2000:])


def test_seed_keys_is_the_yardstick_on_40_phrases_and_hardened_paths_of_every_depth(cli):
    rnd = random.Random(40)
    lens = [1, 2, 111, 112, 127, 128, 129, 215, 259, 260] + [rnd.randrange(1, 261) for _ in range(30)]
    phrases = [bytes(rnd.randrange(33, 127) for _ in range(n)) for n in lens]
    paths = [[rnd.choice((0, 1, 44, 0x7FFFFFFF, rnd.randrange(1 << 31))) | H for _ in range(d)] for d in range(11)]
    text = lambda p: "/".join(["m"] + ["%d%s" % (e & (H - 1), "'h"[i & 1]) for i, e in enumerate(p)])
    for part, pw in ((paths[:6], b""), (paths[6:], b"pass phrase")):
        args = [cli, "seed", "-keys"] + [x for p in part for x in ("-path", text(p))] + (["-pass", pw.decode()] if pw else [])
        pr = subprocess.run(args, input=b"\r\n".join(phrases) + b"\n", capture_output=True, timeout=300)
        assert pr.returncode == 0, pr.stderr
        assert pr.stdout.decode().split() == ["%064x" % R.key_of(ph, p, pw) for ph in phrases for p in part]
    pr = subprocess.run([cli, "seed", "-keys", "-path", "m", "-path", "m/44'/0'/0'"], input=A + b"\n", capture_output=True, timeout=60)
    assert pr.stdout.decode().split() == [TABLE["m"], "fe64af825b5b78554c33a28b23085fc082f691b3c712cc1d4e66e133297da87a"]


def test_seed_keys_past_four_gib_of_input_still_hashes_the_right_bytes(cli):
    """one phrase, 2^32 newlines, then BIP39's test phrase: stdin is read in chunks, so an offset never outgrows the 32 bits a line's
    table entry has for it - the second key is the phrase's master key (the input is newlines: nothing is hashed but the two phrases)"""
    pr = subprocess.Popen([cli, "seed", "-keys", "-path", "m"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    block = b"\n" * (1 << 26)
    pr.stdin.write(b"x\n")
    for _ in range(1 << 6):
        pr.stdin.write(block)
    pr.stdin.write(A)  # (no newline behind the last line)
    pr.stdin.close()
    out = pr.stdout.read().decode().split()
    assert pr.wait(timeout=120) == 0, pr.stderr.read()
    assert out == ["%064x" % R.key_of(b"x", []), TABLE["m"]]


def test_lines_are_cut_as_mul_raw_cuts_them_and_a_path_is_no_other_options_value(cli):
    long = bytes(range(65, 91)) * 100  # 2600 characters: pieces of 1024, 1024 and 552
    feed = b"one\r\n\n\r\n" + long + b"\nlast"
    pr = subprocess.run([cli, "seed", "-keys", "-path", "m/1'"], input=feed, capture_output=True, timeout=60)
    assert pr.returncode == 0 and pr.stdout.decode().split() == ["%064x" % R.key_of(p, [1 | H]) for p in (b"one", long[:1024], long[1024:2048], long[2048:], b"last")]
    # `-pass -path`: the passphrase is the text "-path", and the word behind it is no path
    pr = subprocess.run([cli, "seed", "-keys", "-pass", "-path", "m/x", "-path", "m/2h"], input=b"one\n", capture_output=True, timeout=60)
    assert pr.returncode == 0 and pr.stdout.decode().split() == ["%064x" % R.key_of(b"one", [2 | H], b"-path")], pr.stderr
    pr = subprocess.run([cli, "seed", "-keys", "-path"], input=b"one\n", capture_output=True, timeout=60)
    assert pr.returncode == 1 and b"-path needs a value" in pr.stderr


def test_lines_that_end_on_straddle_and_outgrow_a_chunk_of_stdin(cli):
    """chunks of 1 KiB (ECLOOP_HIP_TEST_SEED_CHUNK): lines of 1 ... 90 bytes over 9 KiB, so many straddle a chunk's end; a newline as a chunk's
    last byte and as the next one's first; a line of 2600 bytes, longer than two chunks, in its pieces of 1024; no newline at the end"""
    rnd = random.Random(1024)
    lines = [bytes(rnd.randrange(33, 127) for _ in range(rnd.randrange(1, 91))) for _ in range(200)]
    head = b"\n".join(lines) + b"\n"
    fill = bytes(rnd.randrange(33, 127) for _ in range(1023 - len(head) % 1024))
    long = bytes(range(65, 91)) * 100
    feed = head + fill + b"\n" + b"\n" + b"after\r\n" + long + b"\nlast"
    assert (len(head) + len(fill) + 1) % 1024 == 0
    want = ["%064x" % R.key_of(p, []) for p in lines + [fill, b"after", long[:1024], long[1024:2048], long[2048:], b"last"]]
    for kib in ("1", "2", "0"):
        pr = subprocess.run([cli, "seed", "-keys", "-path", "m"], input=feed, capture_output=True, timeout=120, env=dict(os.environ, ECLOOP_HIP_TEST_SEED_CHUNK=kib))
        assert pr.returncode == 0 and pr.stdout.decode().split() == want, (kib, pr.stderr)


def test_every_refusal_of_the_command_comes_before_a_gpu_is_looked_for(cli):
    lst = os.path.join(ROOT, "tests", "golden", "btc-puzzles-hash")
    cases = [(["-raw"], "-raw"), (["-bin"], "-bin"), (["-kdf", "keccak"], "-kdf"), (["-p", "1abc"], "-p"), (["-k", "02" + "11" * 32], "-k"), (["-r", "8000:ffff"], "-r"),
             (["-t", "2"], "-t 2"), (["-path", "m/x"], "invalid -path"), (["-path", "44'/0'"], "invalid -path"), (["-path", "m/2147483648"], "invalid -path"),
             (["-path", "m/1//2"], "invalid -path"), (["-path", "m/" + "/".join("1" * 11)], "invalid -path"), (["-path", "m/0"] * 9, "at most 8"),
             (["-pass", "p" * 100], "-pass"), (["-n", "0"], "-n"), (["-n", "1025"], "-n"), (["-n", "x"], "-n"), (["-n", "2", "-path", "m"], "-n"),
             (["-n", "2", "-path", "m/2147483647"], "2^31"), (["-keys", "-path", "m/0"], "hardened"), (["-a", "ce"], "eth is searched alone"), (["-q"], "quiet")]
    for extra, word in cases:
        pr = subprocess.run([cli, "seed", "-f", lst] + extra, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60)
        assert pr.returncode == 1 and pr.stdout == "" and word in pr.stderr, (extra, pr.stderr)
        assert "no MI355X GPU visible" not in pr.stderr, extra
    assert "seed" in subprocess.run([cli], capture_output=True, text=True).stdout


def test_the_bindings_constant_the_header_and_the_record():
    from ecloop_amd import capi
    assert capi.BIP39 == 0x10000 and len(capi.EXPORTS) == 45
    hdr = open(os.path.join(ROOT, "include", "ecloop_hip.h")).read()
    assert re.search(r"#define ECL_KDF_BIP39 0x10000u\b", hdr) and "u32 path[depth]" in hdr
    assert capi.BIP39 & (capi.KDF_CAMP2 | capi.MASK | capi.PREFIX | capi.HERD | capi.INSERT | capi.ORIGIN | capi.PUB | capi.TR | capi.ETH | capi.P2SH | 7) == 0
    rec = capi.Device.seed_record([44 | H, 0, 0xFFFFFFFF], b"pw", reuse=True)
    assert rec == b"B39\0\x01\x03\x02\0" + bytes.fromhex("2c000080" "00000000" "ffffffff") + b"pw" and len(rec) == 8 + 4 * 3 + 2
    assert capi.Device.seed_record([]) == b"B39\0\0\0\0\0"
    d = object.__new__(capi.Device)  # the lines a call is made of, without a library
    d.bip39, seen = True, []
    d.mul_batch_raw = lambda lines, cap=4096: seen.append((lines, cap)) or "result"
    assert d.seed_batch([b"a b", b"c"], [H], passphrase=b"x", cap=7) == "result"
    assert seen == [([b"B39\0\0\x01\x01\0\0\0\0\x80x", b"a b", b"c"], 7)]
    d.bip39 = False
    with pytest.raises(ValueError):
        d.seed_batch([b"a"], [])
    d.h = None
    for kw in (dict(kdf="sha3"), dict(prefix=True), dict(a33=False, eth=True, mask=True), dict(a33=False, pub=True, herd=True), dict(a33=False, pub=True, insert=True),
               dict(a33=False, pub=True, origin=True)):
        with pytest.raises(ValueError):
            capi.Device(0, bip39=True, **kw)


def test_engine_bip39_key_and_parse_path():
    from ecloop_amd import engine
    for path, k in TABLE.items():
        assert "%064x" % engine.bip39_key(A, path) == k
        assert engine.bip39_key(A, engine.parse_path(path)) == int(k, 16) and engine.format_path(engine.parse_path(path)) == path
    assert "%064x" % engine.bip39_key(A, [], b"TREZOR") == "cbedc75b0d6412c85c79bc13875112ef912fd1e756631b5a00330866f22ff184"
    assert engine.parse_path("m/44h/0'/7") == [44 | H, H, 7] and engine.parse_path("m") == []
    rnd = random.Random(7)
    for _ in range(5):
        ph, path = bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 260))), [rnd.randrange(1 << 32) for _ in range(rnd.randrange(4))]
        assert engine.bip39_key(ph, path, b"pw") == R.key_of(ph, path, b"pw")
    for bad in ("44'/0'", "m/", "m/x", "m/-1", "m/2147483648", "m/1'h", "m/" + "/".join("1" * 11), "M/0"):
        with pytest.raises(ValueError):
            engine.parse_path(bad)
    assert "tests" not in open(engine.__file__).read().split("def bip39_key")[1].split("\nclass ")[0]


def test_the_static_figures_of_the_two_kernels():
    """tools/isa_mix.py --seed on the assembly of the shipped code object: k_bip39_master at 128 registers (four waves a SIMD), no scratch
    instruction, call or memory access in the iteration loop - own body plus the two round loops - whose code is far inside the 64 KB
    instruction cache; the figures DESIGN section 7 (f15) states"""
    import sys
    from ecloop_amd.build import build_library
    build_library()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_mix
    r = isa_mix.analyse_seed()
    m, it = r["master"]["registers"], r["master"]["iteration_loop"]
    assert m["vgpr_count"] <= 128 and m["agpr_count"] == 0 and m["group_segment_fixed_size"] == 0
    assert it["scratch"] == 0 and it["calls"] == 0 and it["own"]["vmem"] == 0 and it["own"]["lds"] == 0
    assert all(l["scratch"] == 0 and l["vmem"] == 0 and l["lds"] == 0 for l in it["round_loops"]) and len(it["round_loops"]) == 2
    assert it["code_bytes_max"] < 65536 and it["instructions"] > 2000
    assert 3500 < it["valu_per_compression"] < 4600
    assert abs(it["per_iteration"]["valu"] - 8508) <= 85 and abs(it["floor_phrases_per_s"] - 2598619) <= 26000  # DESIGN's figures, to 1 %
    p = r["path"]["registers"]
    assert p["vgpr_count"] <= 256 and p["vgpr_spill_count"] == 0
