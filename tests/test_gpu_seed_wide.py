"""`seed` on the GPU where tests/test_gpu_seed.py does not go.  What each test reaches that none did before:
  - a call of 2^20 + 65 phrases: seed_batch's SECOND k_bip39_master launch, which reads the table from entry 1 + 2^20 and writes the nodes
    from node 2^20 - every earlier call fits one launch;
  - 2^20 + 50 lines through the host program: cmd_seed's second batch, whose table is rebuilt relative to its own first line and whose hits
    are mapped back through lines[at + key_offset]; -n over a hardened last element;
  - phrases of 0 and of 261 ... 4000 bytes on the device: sha512_text's block loop and the gather from 4 blocks up, the padding spill at
    every block end up to the 8th, the empty HMAC key;
  - seed contexts of -a cu, cus, cu -endo, e -endo, x -endo, which were only opened; a path whose FIRST element is normal (the window sum
    on the master key);
  - add_range, mul_batch and the self-test on a seed context between a fresh call and its reuse = 1 call: the kept nodes survive them;
  - the node buffer's regrow past 1024 entries followed by a smaller fresh call and a reuse of it;
  - the host program for -a e, s, t, x, cu, cs: each type's default path, seed_report's 32-byte keys (p2tr, pub), every type's
    verify_hits branch behind a seed hit.
The expected keys are tests/bip39_ref.py's with the oracle's k G, as in test_gpu_seed.py, whose helpers and fixtures are used here; the
address of a key is eth_ref's, tr_ref's, p2sh_ref's, pub_ref's or the oracle's.  Every comparison is exact.  Every subprocess that opens
the GPU runs under its own `timeout -k 10`."""
import ctypes as C
import random

import numpy as np
import pytest

import bip39_ref as R
import eth_ref
import orc
import p2sh_ref
import pub_ref
import tr_ref
from support import SEED_LONG_LENS, cli, counts, rec_set, run_cli
from test_gpu_seed import BIP44, H, ONES, check, key, key_of, pair, phrases64

pytestmark = pytest.mark.gpu
M = 1 << 20  # SEED_MASTER_LAUNCH (csrc/abi_seed.h) and SEED_BATCH (host/cli_seed.h)


def test_a_call_of_two_master_launches(pair, phrases64):
    """2^20 + 65 lines, line i = phrase i % 61: 2^20 % 61 = 47, so the second launch's 65 lines - one whole wave and one lane of a second
    block - differ from lines 0 ... 64 and from their neighbours; a launch that restarts at line 0 or is off by one entry changes records.
    Then the same nodes by reuse = 1 at the next index."""
    from ecloop_amd import capi
    d, plain = pair
    ph = phrases64[:61]
    np_ = M + 65
    assert len(set(ph)) == 61 and M % 61 == 47
    rec = d.seed_record(BIP44)
    text = rec + b"".join(ph)
    starts = np.cumsum([len(rec)] + [len(p) for p in ph])[:-1].astype(np.uint64)
    one = starts | (np.array([len(p) for p in ph], dtype=np.uint64) << np.uint64(32))
    table = np.concatenate([[np.uint64(len(rec)) << np.uint64(32)], one[np.arange(np_) % 61]]).astype(np.uint64)
    out = np.zeros(np_ + 8, dtype=capi.FOUND_DTYPE)
    cnt = C.c_uint32()
    for last, reuse in ((0, False), (1, True)):
        path = BIP44[:4] + [last]
        head = d.seed_record(path, reuse=reuse)
        assert len(head) == len(rec)
        buf = np.frombuffer(head + text[len(rec):], dtype=np.uint8)
        ref, n = plain.mul_batch([key_of(p, path) for p in ph], cap=64)
        assert n == 61
        want = np.zeros((61, 5), np.uint32)
        want[ref["key_offset"].astype(np.int64)] = ref["h160"]
        cov = d.coverage()
        assert d.lib.ecl_hip_mul_batch_raw(d.h, buf.ctypes.data, len(text), table.ctypes.data, np_ + 1, out.ctypes.data, np_ + 8, C.byref(cnt)) == 0
        assert cnt.value == np_ and tuple(b - a for a, b in zip(cov, d.coverage())) == (np_, np_, np_), reuse
        got = out[:np_]
        assert np.array_equal(np.sort(got["key_offset"]), np.arange(np_)), reuse
        assert np.array_equal(got["h160"], want[got["key_offset"].astype(np.int64) % 61]) and (got["compressed"] == 1).all(), reuse


def test_two_batches_through_the_host_program(cli, tmp_path):
    """2^20 + 50 distinct lines, two paths, -n 3, a passphrase: planted keys on the first and the last line of each batch, at the first
    path's indexes 0 and 2 and at the second path's hardened last elements 7' and 9'.  A hit of the second batch mapped to a line of the
    first fails the program's own re-derivation (hash mismatch, exit status 1)."""
    nl = M + 50
    first, second = "m/44'/0'/0'/0/%d", "m/0'/%d'"
    plan = [(0, first % 0), (M - 1, second % 9), (M, first % 2), (M + 49, second % 7)]
    want, hs = [], []
    for i, p in plan:
        k = key_of(b"w%07d" % i, R.path_of(p), b"pw")
        hs.append(orc.hex160(orc.hash160(*orc.point_of(k), True)))
        want.append("addr33\t%s\t%064x\t%s\tw%07d" % (hs[-1], k, p, i))
    lst = tmp_path / "list.txt"
    lst.write_text("".join(h + "\n" for h in hs))
    ph = tmp_path / "phrases.txt"
    ph.write_bytes(b"".join(b"w%07d\n" % i for i in range(nl)))
    r = run_cli(cli, ["seed", "-f", str(lst), "-path", first % 0, "-path", "m/0'/7h", "-n", "3", "-pass", "pw"], stdin_path=str(ph),
                out=str(tmp_path / "found"), hard_limit=300, check=False)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.lines == sorted(want)
    assert counts(r.status) == (4, 6291756) and nl * 2 * 3 == 6291756, r.status


def test_phrases_of_0_and_of_261_to_4000_bytes_at_mixed_alignments(pair):
    rnd = random.Random(4000)
    phrases = [bytes(rnd.randrange(256) for _ in range(n)) for n in SEED_LONG_LENS]
    assert len(phrases) == 154 and len(phrases[0]) == 0 and len(phrases[-1]) == 4000
    starts = np.cumsum([14] + [len(p) for p in phrases])[:-1]  # (behind the record: 8 + 4 + 2 bytes)
    assert {int(s) & 3 for s in starts} == {0, 1, 2, 3}
    check(pair, phrases, [7 | H], b"pw")


SELECTIONS = {"cu": (dict(a33=True, a65=True), {0, 1}), "cus": (dict(a33=True, a65=True, p2sh=True), {0, 1, 2}), "cu-endo": (dict(a33=True, a65=True, endo=True), {0, 1}),
              "e-endo": (dict(a33=False, eth=True, endo=True), {3}), "x-endo": (dict(a33=False, pub=True, endo=True), {5})}


@pytest.mark.parametrize("ctx", list(SELECTIONS))
def test_combined_selections_and_endo_contexts(ctx, phrases64):
    """40 phrases at BIP44 and at m/0/5' - a normal FIRST element: the window sum runs on the master key - on a seed context of each
    selection: the records (offset, endo, type, hash) of mul_batch over the yardstick's keys on a context with the same flags"""
    from ecloop_amd import Device
    kw, types = SELECTIONS[ctx]
    ph = phrases64[:40]
    d, plain = Device(0, bip39=True, **kw), Device(0, **kw)
    try:
        d.set_bloom(ONES), plain.set_bloom(ONES)
        for path in (BIP44, [0, 5 | H]):
            want_k = [key_of(p, path) for p in ph]
            assert all(want_k)
            got, n = d.seed_batch(ph, path, cap=256)
            ref, n2 = plain.mul_batch(want_k, cap=256)
            assert n == n2 == 40 * len(types) and rec_set(got) == rec_set(ref), path
            assert not got["endo"].any() and set(got["compressed"].tolist()) == types, path
    finally:
        d.close(), plain.close()


def grows(d, before, by):
    now = d.coverage()
    assert tuple(b - a for a, b in zip(before, now)) == (by, by, by), (before, now, by)
    return now


def test_the_kept_nodes_survive_add_range_mul_batch_and_the_selftest(pair, phrases64):
    d, plain = pair
    ph = phrases64[:24]
    cov = d.coverage()
    check(pair, ph, BIP44)
    cov = grows(d, cov, 24)
    got, n = d.add_range(0x800000, 4096, cap=8192)
    ref, n2 = plain.add_range(0x800000, 4096, cap=8192)
    assert n == n2 == 4096 and rec_set(got) == rec_set(ref)
    cov = grows(d, cov, 4096)
    rnd = random.Random(100)
    ks = [rnd.randrange(1, orc.N) for _ in range(100)]
    got, n = d.mul_batch(ks, cap=128)
    ref, n2 = plain.mul_batch(ks, cap=128)
    assert n == n2 == 100 and key(got) == key(ref)
    cov = grows(d, cov, 100)
    assert d.lib.ecl_hip_selftest(d.h) == 0 and plain.lib.ecl_hip_selftest(plain.h) == 0
    cov = grows(d, cov, 0)  # (the self-test leaves the totals "since open" as they were)
    check(pair, ph, BIP44[:4] + [1], reuse=True)
    grows(d, cov, 24)


def test_the_node_buffer_regrows_and_a_smaller_call_and_its_reuse_follow(phrases64):
    """a fresh context keeps 1024 nodes: 24 phrases, then 1500 (the buffer grows), then 24 OTHER phrases, then reuse = 1, which serves those"""
    from ecloop_amd import Device
    d, plain = Device(0, a33=True, bip39=True), Device(0, a33=True)
    try:
        d.set_bloom(ONES), plain.set_bloom(ONES)
        check((d, plain), phrases64[:24], BIP44)
        check((d, plain), [b"n%04d" % i for i in range(1500)], [H])
        check((d, plain), phrases64[24:48], BIP44)
        check((d, plain), phrases64[24:48], BIP44[:4] + [1], reuse=True)
    finally:
        d.close(), plain.close()


def address_lines(types, k):
    """the found lines' heads, "label: address <- key", of the private key k for a selection"""
    x, y = orc.point_of(k)
    h33 = orc.hex160(orc.hash160(x, y, True))
    heads = {"c": "addr33: " + h33, "u": "addr65: " + orc.hex160(orc.hash160(x, y, False)), "s": "p2sh: " + p2sh_ref.p2sh_hex(h33),
             "e": "eth: " + eth_ref.eth_hex(x, y), "t": "p2tr: %064x" % tr_ref.output_key(k), "x": "pub: " + pub_ref.compressed(k)}
    return ["%s <- %064x" % (heads[t], k) for t in types]


DEFAULT_PATH = {"e": "m/44'/60'/0'/0/0", "s": "m/49'/0'/0'/0/0", "t": "m/86'/0'/0'/0/0", "x": "m/44'/0'/0'/0/0", "cu": "m/44'/0'/0'/0/0", "cs": "m/44'/0'/0'/0/0"}


@pytest.mark.parametrize("types", list(DEFAULT_PATH))
def test_the_host_program_at_the_default_path_of_every_selection(cli, tmp_path, phrases64, types):
    """`seed -a <types>` with no -path: 50 phrases, a list in the type's own line format - 0x addresses, 64 digits of an output key, 66-digit
    keys, hash160s - that holds phrase 7 with every address of the selection and phrase 41 with the selection's last one; the found lines
    are the yardstick's: label, address (p2tr: all 32 bytes; pub: the compressed key), key, the default path's text, phrase"""
    phrases = phrases64[:50]
    path = DEFAULT_PATH[types]
    want = []
    for i, which in ((7, types), (41, types[-1])):
        want += ["%s %s %s" % (l, path, phrases[i].decode()) for l in address_lines(which, key_of(phrases[i], R.path_of(path)))]
    lst = tmp_path / "list.txt"
    lst.write_text("".join(("0x" if types == "e" else "") + w.split()[1] + "\n" for w in want))
    ph = tmp_path / "phrases.txt"
    ph.write_bytes(b"\n".join(phrases) + b"\n")
    r = run_cli(cli, ["seed", "-f", str(lst), "-a", types], stdin_path=str(ph), hard_limit=120, check=False)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.found == sorted(want), r.stdout
    assert counts(r.status) == (len(want), 50), r.status
