"""Ethereum addresses (`-a e`, ECL_ETH) on the GPU: known answers and the flag rules through the C ABI, every key x endo image of a range
through an all-ones filter against tests/eth_ref.py (a pure-Python Keccak-256 over the oracle's points), addr65 unchanged beside it, the
CLI's found lines (0x list, .blf, -endo), `mul` / `mul -raw` / `rnd`, key coverage, and the look-ahead keeping ETH and addr65 contexts
apart.  Every GPU-using subprocess runs under its own time limit."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import eth_ref
import orc
from support import GOLD, cli, counts, rec_set, run_cli
from synth import synth_bloom_words

pytestmark = pytest.mark.gpu
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
KNOWN = {1: "7e5f4552091a69125d5dfcb7b8c2659029395bdf", 2: "2b5ad5c4795c026514f8317c7a215e218dccd6cf",
         0xdc2a04: "d2c71c0b28f045d0e6facc19a3a6a81a85a17ce4", 0x8000: "8af7c4e8e5f28db7cd19ad12818458d73547d2ec",
         0xffffff: "1c68cf50fac5639f9fd70946be6c2fcfdff19f33"}
RANGES = [(0x3F000, 3000, 0), (0x123456789ABCDEF, 1500, 7)]


def eth_of(k):
    return eth_ref.eth_hex(*orc.point_of(k))


def test_abi_known_answers_and_flags():
    from ecloop_amd import Device, capi
    d = Device(0, a33=False, eth=True)  # (the self-test runs its walk cross-check with ETH addresses)
    try:
        addr, ok = d.verify_eth(list(KNOWN) + [0, orc.N])
        assert [orc.hex160(a) for a in addr[:len(KNOWN)]] == list(KNOWN.values())
        assert [int(v) for v in ok] == [1] * len(KNOWN) + [0, 0]
    finally:
        d.close()
    d = Device(0)  # any context can be asked
    try:
        addr, ok = d.verify_eth(list(KNOWN))
        assert [orc.hex160(a) for a in addr] == list(KNOWN.values()) and ok.all()
    finally:
        d.close()
    lib = capi.load()
    for flags in (capi.ETH | capi.ADDR33, capi.ETH | capi.ADDR65, capi.ETH | capi.P2SH, capi.ETH | 8, capi.ETH | 32,
                  capi.ETH | capi.ADDR33 | capi.ENDO):
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, flags, 0) == -1, flags  # ECL_E_ARG: eth is searched alone; 8 and 32 stay unknown bits
    for flags in (capi.ETH, capi.ETH | capi.ENDO):
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, flags, 0) == 0, flags
        lib.ecl_hip_close(h)
    with pytest.raises(ValueError):
        Device(0, eth=True)  # a33 defaults to True: any other type beside eth raises before the library is asked


def all_records(endo, start, nkeys, offs, **types):
    from ecloop_amd import Device
    d = Device(0, endo=endo, ord_offs=offs, **types)
    try:
        d.set_bloom(ONES)
        before = d.coverage()
        cap = nkeys * (6 if endo else 1)
        recs, n = d.add_range(start, nkeys, cap=cap + 16)
        assert n == len(recs)
        after = d.coverage()
        return recs, tuple(b - a for a, b in zip(before, after))
    finally:
        d.close()


@pytest.mark.parametrize("endo", [False, True], ids=["plain", "endo"])
@pytest.mark.parametrize("start,nkeys,offs", RANGES, ids=["contiguous", "stride128"])
def test_every_key_and_image_once_with_the_right_address(endo, start, nkeys, offs):
    """all-ones filter: exactly one record per key x image, all of type 3, each address the yardstick's for the point of
    calc_priv(start, stride, offset, endo) - the oracle's point, the pure-Python Keccak; the call's coverage totals grow by its keys;
    and an addr65 context gives the same records before and after an ETH context lived in the process (negative control)"""
    from ecloop_amd.engine import calc_priv
    imgs = 6 if endo else 1
    u_before, _ = all_records(endo, start, nkeys, offs, a33=False, a65=True)
    recs, grown = all_records(endo, start, nkeys, offs, a33=False, eth=True)
    u_after, _ = all_records(endo, start, nkeys, offs, a33=False, a65=True)
    got = [(int(r["key_offset"]), int(r["endo"])) for r in recs]
    assert len(got) == len(set(got)) == nkeys * imgs
    assert set(got) == {(off, e) for off in range(nkeys) for e in range(imgs)}
    assert all(int(r["compressed"]) == 3 for r in recs)
    assert grown == (nkeys, nkeys, nkeys)  # requested == covered == counted on the device
    for (off, e), r in zip(got, recs):
        k = calc_priv(start, 1 << offs, off, e)
        assert [int(v) for v in r["h160"]] == eth_ref.eth_words(*orc.point_of(k)), (off, e)
    assert rec_set(u_before) == rec_set(u_after) and len(u_before) == nkeys * imgs
    assert all(int(r["compressed"]) == 0 for r in u_after)


def test_drop_round_fails_an_eth_call():
    from ecloop_amd import Device, EclError
    d = Device(0, a33=False, eth=True)
    try:
        d.set_bloom(synth_bloom_words(4099, 3, "a|b"))
        d.set_lookahead(0)
        d.set_geometry(8, 256)
        n = 1 << 17
        d.add_range(0x7_0000_0000, n)
        cov = d.coverage()
        d.diag_drop_round()
        with pytest.raises(EclError) as e:
            d.add_range(0x7_0000_0000 + n, n)
        assert e.value.code == -8
        now = d.coverage()
        assert now[0] - cov[0] == n and now[1] == cov[1] and now[2] - cov[2] < n
        recs, total = d.add_range(0x7_0000_0000 + n, n)  # whole again
        assert total == len(recs)
        after = d.coverage()
        assert after[0] - now[0] == after[1] - now[1] == after[2] - now[2] == n
    finally:
        d.close()


def test_cli_add_finds_the_eth_lines_from_a_0x_list_and_a_blf(cli, tmp_path):
    lst = tmp_path / "eth.txt"
    lst.write_text("0x%s\n0x%s\n" % (KNOWN[0xdc2a04], KNOWN[0xffffff]))
    want = sorted("eth: %s <- %064x" % (KNOWN[k], k) for k in (0xdc2a04, 0xffffff))
    r = run_cli(cli, ["add", "-f", str(lst), "-a", "e", "-r", "800000:ffffff"])
    assert r.found == want and counts(r.status) == (2, 8388608), (r.stdout, r.status)
    assert "~ endo: 0 ~ eth: 1 | filter: list (2)" in r.stdout
    r = run_cli(cli, ["add", "-f", str(lst), "-a", "e", "-r", "800000:ffffff"], env={"ECLOOP_HIP_STATS": "1"})
    assert r.found == want and "list: 2 entries" in r.stderr  # both 0x lines were read
    assert re.search(r"coverage: requested 8388608, covered 8388608, device \d+", r.stdout), r.stdout
    blf = str(tmp_path / "eth.blf")
    subprocess.run([cli, "blf-gen", "-a", "e", "-n", "1000", "-o", blf], stdin=open(str(lst), "rb"), stdout=subprocess.PIPE, check=True, timeout=120)
    r = run_cli(cli, ["add", "-f", blf, "-a", "e", "-r", "800000:ffffff"])
    assert "filter: bloom" in r.stdout and r.found == want and counts(r.status) == (2, 8388608)
    r = run_cli(cli, ["add", "-f", str(lst), "-a", "e", "-endo", "-r", "800000:ffffff"])
    assert r.found == want and counts(r.status) == (2, 8388608 * 6) and "~ endo: 1 ~ eth: 1 |" in r.stdout
    # without -a e the same file holds no entry
    pr = subprocess.run([cli, "add", "-f", str(lst), "-r", "800000:ffffff"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=120)
    assert pr.returncode != 0 and "no hashes in filter file" in pr.stderr


def test_mul_mul_raw_and_rnd_report_the_planted_addresses(cli, tmp_path):
    lines = [l.strip() for l in open(os.path.join(GOLD, "mul_scalars.txt")) if l.strip()]
    picked = [lines[i] for i in (3, 77, 200)]
    phrases = [b"eth test phrase", b"correct horse battery staple", b"keccak not sha3"]
    others = [b"phrase %d" % i for i in range(2000)]
    pk_of_phrase = lambda p: int.from_bytes(hashlib.sha256(p).digest(), "big")
    planted = ["eth: %s <- %064x" % (eth_of(k), k) for k in [orc.sn_from_hex(l) for l in picked] + [pk_of_phrase(p) for p in phrases]]
    lst = tmp_path / "planted.txt"
    lst.write_text("".join("0x" + l.split()[1] + "\n" for l in planted))
    r = run_cli(cli, ["mul", "-f", str(lst), "-a", "e"], stdin_path=os.path.join(GOLD, "mul_scalars.txt"))
    assert r.found == sorted(planted[:3]), r.stdout
    assert "~ eth: 1 |" in r.stdout
    ph = tmp_path / "phrases.txt"
    ph.write_bytes(b"\n".join(others[:1000] + phrases + others[1000:]) + b"\n")
    r = run_cli(cli, ["mul", "-raw", "-f", str(lst), "-a", "e"], stdin_path=str(ph))
    assert r.found == sorted(planted[3:]), r.stdout
    one = tmp_path / "dc.txt"
    one.write_text("0x%s\n" % KNOWN[0xdc2a04])
    r = run_cli(cli, ["rnd", "-f", str(one), "-a", "e", "-seed", "eth", "-r", "800000:ffffff", "-d", "0:23"])
    assert r.found == ["eth: %s <- %064x" % (KNOWN[0xdc2a04], 0xdc2a04)], r.stdout


def test_lookahead_keeps_eth_and_addr65_contexts_apart():
    """two contexts on the same filter, one `-a u`, one `-a e`, each walking the reference's pattern of small contiguous jobs: each runs its own
    sweeps (different flags = different look-ahead groups) and receives exactly the records of its own type that a plain launch gives"""
    from ecloop_amd import Device
    words = synth_bloom_words(4099, 3, "a|b")  # passes one hash in ~300
    A, job, jobs = 0x300000000, 1 << 21, 24  # the reference's job size (MAX_JOB_SIZE): ~7000 records per job with this filter
    mk = {"u": lambda: Device(0, a33=False, a65=True), "e": lambda: Device(0, a33=False, eth=True)}
    ctx = {t: f() for t, f in mk.items()}
    plain = {t: f() for t, f in mk.items()}
    try:
        for d in list(ctx.values()) + list(plain.values()):
            d.set_bloom(words)
        for d in plain.values():
            d.set_lookahead(0)
        for d in ctx.values():
            d.set_lookahead(1 << 26)
            d.set_scan_end(A + jobs * job)
        mine = {"u": [], "e": []}
        for j in range(jobs):
            for t, d in ctx.items():  # interleaved, as two worker threads would call
                recs, n = d.add_range(A + j * job, job, cap=1 << 15)
                assert n == len(recs)
                mine[t] += [(A + j * job + int(r["key_offset"]), int(r["compressed"]), orc.hex160(r["h160"])) for r in recs]
        for t, want_type in (("u", 0), ("e", 3)):
            recs, n = plain[t].add_range(A, jobs * job, cap=1 << 19)
            assert n == len(recs)
            ref = sorted((A + int(r["key_offset"]), int(r["compressed"]), orc.hex160(r["h160"])) for r in recs)
            assert sorted(mine[t]) == ref and ref and all(x[1] == want_type for x in ref), t
            sweeps, _, served, _ = ctx[t].lookahead_stats()
            # by the header's rules the first job of a pattern is always launched plainly, and a remainder of fewer than 4 jobs is never
            # swept: everything else must have been answered from a sweep
            assert sweeps >= 1 and served >= jobs - 4, (t, sweeps, served)
        for k, _, h in [x for x in mine["e"]][:32]:  # ... and what the sweeps reported are Ethereum addresses
            assert h == eth_of(k)
    finally:
        for d in list(ctx.values()) + list(plain.values()):
            d.close()
