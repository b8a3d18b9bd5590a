"""P2SH-P2WPKH (nested SegWit, BIP49 "3..." addresses; `-a s`, ECL_P2SH) on the GPU: known answers through the C ABI, every key x type x
endo image of a range through an all-ones filter against hash160(0x00 0x14 || the oracle's addr33 hash), the other types unchanged beside
it, the CLI's found lines (list, .blf, -o, two contexts), `mul` / `mul -raw`, and the look-ahead keeping P2SH and addr33 contexts apart."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import orc
import p2sh_ref
from support import GOLD, cli, counts, rec_set, run_cli
from synth import synth_bloom_words

pytestmark = pytest.mark.gpu
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
KEY_DC = 0xDC2A04
P2SH_DC = "45a41e75045f683ed5f71fec4b4322fcd263891b"
KNOWN = {1: "bcfeb728b584253d5f3f70bcb780e9ef218a68f4", 2: "978a0121f9a24de65a13bab0c43c3a48be074eae", KEY_DC: P2SH_DC}
TYPES = {"c": dict(a33=True, a65=False, p2sh=False), "u": dict(a33=False, a65=True, p2sh=False), "cu": dict(a33=True, a65=True, p2sh=False),
         "s": dict(a33=False, a65=False, p2sh=True), "cs": dict(a33=True, a65=False, p2sh=True), "us": dict(a33=False, a65=True, p2sh=True),
         "cus": dict(a33=True, a65=True, p2sh=True)}


def h33_of(k):
    x, y = orc.point_of(k)
    return orc.hash160(x, y, True)


def test_abi_known_answers_and_flags():
    from ecloop_amd import Device, capi
    d = Device(0, a33=False, p2sh=True)  # P2SH alone is a valid type set (the self-test runs its walk cross-check with it)
    try:
        got = d.p2sh_hash([h33_of(k) for k in KNOWN])
        assert [orc.hex160(g) for g in got] == list(KNOWN.values())
    finally:
        d.close()
    lib = capi.load()
    for flags in (8, 32, capi.P2SH | 8, capi.P2SH | 32, capi.ENDO):
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, flags, 0) == -1, flags  # ECL_E_ARG: an unknown bit, or no address type


def all_records(types, endo, start, nkeys, offs):
    from ecloop_amd import Device
    d = Device(0, endo=endo, ord_offs=offs, **TYPES[types])
    try:
        d.set_bloom(ONES)
        cap = nkeys * len(types) * (6 if endo else 1)
        recs, n = d.add_range(start, nkeys, cap=cap + 16)
        assert n == len(recs)
        return recs
    finally:
        d.close()


@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
@pytest.mark.parametrize("start,nkeys,offs", [(0x3F000, 3000, 0), (0x123456789ABCDEF, 1500, 7)], ids=["contiguous", "stride128"])
def test_every_key_type_and_image_once_with_the_right_hash(endo, start, nkeys, offs):
    """all-ones filter: every key x type x image is reported exactly once; P2SH records carry the script hash of the oracle's addr33 hash of
    calc_priv(key, endo), the addr33 / addr65 records the oracle's hashes; a context without P2SH reports the same addr33 / addr65 records
    (negative control: adding `s` changes nothing else)"""
    from ecloop_amd.engine import calc_priv
    imgs = 6 if endo else 1
    keys = {(off, e): calc_priv(start, 1 << offs, off, e) for off in range(nkeys) for e in range(imgs)}
    K = np.array([[(k >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for k in keys.values()], np.uint64)
    h33, h65, ok = orc.mul_hash160_many(K, a33=True, a65=True)
    assert ok.all()
    want = {}
    for j, ke in enumerate(keys):
        want[ke + (1,)] = [int(v) for v in h33[j]]
        want[ke + (0,)] = [int(v) for v in h65[j]]
        want[ke + (2,)] = p2sh_ref.p2sh_of_h33(h33[j])
    for types in ("s", "cs", "us", "cus"):
        recs = all_records(types, endo, start, nkeys, offs)
        kinds = {"c": 1, "u": 0, "s": 2}
        wanted_types = {kinds[t] for t in types}
        got = [(int(r["key_offset"]), int(r["endo"]), int(r["compressed"])) for r in recs]
        assert len(got) == len(set(got)) == nkeys * imgs * len(types), types
        assert set(got) == {ke + (t,) for ke in keys for t in wanted_types}, types
        for g, r in zip(got, recs):
            assert [int(v) for v in r["h160"]] == want[g], (types, g)
        # the same call without P2SH: identical addr33 / addr65 records
        if types != "s":
            base = all_records(types.replace("s", ""), endo, start, nkeys, offs)
            assert rec_set(base) == rec_set([r for r in recs if int(r["compressed"]) != 2]), types


@pytest.fixture(scope="module")
def hash_list(tmp_path_factory):
    p = tmp_path_factory.mktemp("p2shlist") / "puzzles-and-p2sh.txt"
    p.write_text(open(os.path.join(GOLD, "btc-puzzles-hash")).read().rstrip("\n") + "\n" + P2SH_DC + "\n")
    return str(p)


def test_cli_add_finds_the_p2sh_line(cli, hash_list, tmp_path):
    key = "%064x" % KEY_DC
    addr33 = "addr33: %s <- %s" % (orc.hex160(h33_of(KEY_DC)), key)
    p2sh = "p2sh: %s <- %s" % (P2SH_DC, key)
    for env in ({}, {"ECLOOP_HIP_SHARE_GPU": "2"}):
        r = run_cli(cli, ["add", "-f", hash_list, "-a", "s", "-r", "800000:ffffff"], env=env)
        assert r.found == [p2sh] and counts(r.status) == (1, 8388608), (env, r.stdout, r.status)
        assert "~ endo: 0 ~ p2sh: 1 | filter: list" in r.stdout
        r = run_cli(cli, ["add", "-f", hash_list, "-a", "cs", "-r", "800000:ffffff"], env=env)
        assert r.found == sorted([addr33, p2sh]) and counts(r.status) == (2, 8388608), (env, r.stdout, r.status)
        f = str(tmp_path / ("o%d.txt" % len(env)))
        r = run_cli(cli, ["add", "-f", hash_list, "-a", "cs", "-r", "800000:ffffff"], out=f, env=env)
        assert sorted(open(f).read().splitlines()) == sorted([addr33.replace(": ", "\t").replace(" <- ", "\t"), "p2sh\t%s\t%s" % (P2SH_DC, key)])
        assert counts(r.status) == (2, 8388608)
    # without `s` the banner is the one it always was
    r = run_cli(cli, ["add", "-f", hash_list, "-a", "c", "-r", "800000:ffffff"])
    assert r.found == [addr33] and "p2sh" not in r.stdout and "~ endo: 0 | filter: list" in r.stdout


def test_list_mode_and_blf_give_the_same_p2sh_records(cli, hash_list, tmp_path):
    """the device list confirm (ecl_hip_set_list) keeps a P2SH hit; a .blf made by blf-gen from the same list finds the same line"""
    from ecloop_amd import Device
    from ecloop_amd.engine import load_filter
    flt = load_filter(hash_list)
    d = Device(0, a33=False, p2sh=True)
    try:
        d.set_bloom(flt.words)
        d.set_list(flt.hashes)
        recs, n = d.add_range(0x800000, 0x800000, cap=64)
    finally:
        d.close()
    got = sorted("p2sh: %s <- %064x" % (orc.hex160(r["h160"]), 0x800000 + int(r["key_offset"])) for r in recs if int(r["compressed"]) == 2)
    assert n == 1 and got == ["p2sh: %s <- %064x" % (P2SH_DC, KEY_DC)]
    blf = str(tmp_path / "l.blf")
    subprocess.run([cli, "blf-gen", "-n", "1000000", "-o", blf], stdin=open(hash_list, "rb"), stdout=subprocess.PIPE, check=True)
    r = run_cli(cli, ["add", "-f", blf, "-a", "s", "-r", "800000:ffffff"])
    assert "filter: bloom" in r.stdout and r.found == got and counts(r.status) == (1, 8388608)


def test_mul_and_mul_raw_report_the_planted_script_hashes(cli, tmp_path):
    lines = [l.strip() for l in open(os.path.join(GOLD, "mul_scalars.txt")) if l.strip()]
    picked = [lines[i] for i in (3, 77, 200)]
    phrases = [b"p2sh test phrase", b"correct horse battery staple", b"nested segwit"]
    others = [b"phrase %d" % i for i in range(500)]
    pk_of_phrase = lambda p: int.from_bytes(hashlib.sha256(p).digest(), "big")
    planted = {}
    for l in picked:
        k = orc.sn_from_hex(l)
        planted["p2sh: %s <- %064x" % (p2sh_ref.p2sh_hex(orc.hex160(h33_of(k))), k)] = None
    for p in phrases:
        k = pk_of_phrase(p)
        planted["p2sh: %s <- %064x" % (p2sh_ref.p2sh_hex(orc.hex160(h33_of(k))), k)] = None
    lst = tmp_path / "planted.txt"
    lst.write_text("".join(l.split()[1] + "\n" for l in planted))
    r = run_cli(cli, ["mul", "-f", str(lst), "-a", "s"], stdin_path=os.path.join(GOLD, "mul_scalars.txt"))
    assert r.found == sorted(list(planted)[:3]), r.stdout
    assert "~ p2sh: 1 |" in r.stdout
    ph = tmp_path / "phrases.txt"
    ph.write_bytes(b"\n".join(others[:250] + phrases + others[250:]) + b"\n")
    r = run_cli(cli, ["mul", "-raw", "-f", str(lst), "-a", "s"], stdin_path=str(ph))
    assert r.found == sorted(list(planted)[3:]), r.stdout
    # `-a cs`: the addr33 hashes of the same scalars are not in the list, so the same lines come back
    r = run_cli(cli, ["mul", "-f", str(lst), "-a", "cs"], stdin_path=os.path.join(GOLD, "mul_scalars.txt"))
    assert r.found == sorted(list(planted)[:3])


def test_lookahead_keeps_p2sh_and_addr33_contexts_apart():
    """two contexts on the same filter, one `-a c`, one `-a s`, each walking the reference's pattern of small contiguous jobs: each runs its own
    sweeps (different flags = different look-ahead groups) and receives exactly the records of its own type that a plain launch gives"""
    from ecloop_amd import Device
    words = synth_bloom_words(4099, 3, "a|b")  # passes one hash in ~300
    A, job, jobs = 0x300000000, 1 << 14, 24
    ctx = {"c": Device(0, a33=True), "s": Device(0, a33=False, p2sh=True)}
    plain = {"c": Device(0, a33=True), "s": Device(0, a33=False, p2sh=True)}
    try:
        for d in list(ctx.values()) + list(plain.values()):
            d.set_bloom(words)
        for d in plain.values():
            d.set_lookahead(0)
        for d in ctx.values():
            d.set_lookahead(1 << 22)
            d.set_scan_end(A + jobs * job)
        mine = {"c": [], "s": []}
        for j in range(jobs):
            for t, d in ctx.items():  # interleaved, as two worker threads would call
                recs, n = d.add_range(A + j * job, job, cap=4096)
                assert n == len(recs)
                mine[t] += [(A + j * job + int(r["key_offset"]), int(r["compressed"]), orc.hex160(r["h160"])) for r in recs]
        for t, want_type in (("c", 1), ("s", 2)):
            recs, n = plain[t].add_range(A, jobs * job, cap=1 << 16)
            ref = sorted((A + int(r["key_offset"]), int(r["compressed"]), orc.hex160(r["h160"])) for r in recs)
            assert sorted(mine[t]) == ref and ref and all(x[1] == want_type for x in ref), t
            sweeps, _, served, _ = ctx[t].lookahead_stats()
            assert sweeps >= 1 and served >= jobs - 2, (t, sweeps, served)
    finally:
        for d in list(ctx.values()) + list(plain.values()):
            d.close()
