"""Taproot (`-a t`, ECL_TR) on the GPU: known answers and the flag rules through the C ABI, every key of two ranges through an all-ones
filter against tests/tr_ref.py (pure-Python BIP341 over the oracle's points), slabs of any size giving the same records, overflow and
fetch, list mode, `mul` / `mul -raw`, both coverage counts, the look-ahead, and the CLI's found lines.  Every GPU-using subprocess runs
under its own time limit."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import orc
import tr_ref
from support import GOLD, ROOT, cli, counts, rec_set, run_cli
from synth import synth_bloom_words

pytestmark = pytest.mark.gpu
ONES = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
V1_X = 0xd6889cb081036e0faefa3a35157ad71086b123b2b144b649798b494c300a961d
V1_T = 0xb86e7be8f39bab32a6f2c0443abbc210f0edac0e2c53d501b36b64437d9c6c70
V1_Q = 0x53a1f6e454df1aa2776a2814a721372d6258050de330b3c6d10ee8f4e0dda343
KNOWN = {1: 0xda4710964f7852695de2da025290e24af6d8c281de5a0b902b7135fd9fd74d21,
         2: 0xcafd90c7026f0b6ab98df89490d02732881f2f4b5900856358dddff4679c2ffb,
         0xdc2a04: 0x509eeff5f103f2767a17d3289d857dd538a62a9449646107e5b4b6d0a7898714}
RANGES = [(0x3F000, 3000, 0), (0x123456789ABCDEF, 1500, 7)]  # the ranges of tests/test_gpu_eth.py


def key_of(words):
    return sum(int(w) << (32 * (7 - i)) for i, w in enumerate(words))


def h160_of(k):
    return tuple(tr_ref.words5(tr_ref.output_key(k)))


def tr_device(words=ONES, offs=0, lookahead=0):
    from ecloop_amd import Device
    d = Device(0, a33=False, tr=True, ord_offs=offs)
    d.set_bloom(words)
    d.set_lookahead(lookahead)
    return d


def test_abi_known_answers_and_flags():
    from ecloop_amd import Device, capi
    d = Device(0, a33=False, tr=True)  # (the self-test runs its walk cross-check with output keys)
    try:
        qx, ok = d.verify_tr(list(KNOWN) + [0, orc.N])
        assert [key_of(q) for q in qx[:3]] == list(KNOWN.values())
        assert [int(v) for v in ok] == [1, 1, 1, 0, 0]
        y = pow(V1_X ** 3 + 7, (orc.P + 1) // 4, orc.P)
        pts = [(V1_X, y), (V1_X, orc.P - y)] + [orc.point_of(k) for k in KNOWN]
        t, qx, ok = d.diag_tr([p[0] for p in pts], [p[1] for p in pts])  # the BIP341 vector on the device code of the search path
        assert t[0] == t[1] == V1_T and key_of(qx[0]) == key_of(qx[1]) == V1_Q and ok.all()
        assert [key_of(q) for q in qx[2:]] == list(KNOWN.values())
    finally:
        d.close()
    d = Device(0)  # any context can be asked
    try:
        qx, ok = d.verify_tr(list(KNOWN))
        assert [key_of(q) for q in qx] == list(KNOWN.values()) and ok.all()
    finally:
        d.close()
    lib = capi.load()
    for other in (1, 2, 4, 8, 16, 32, 64):
        h = C.c_void_p()
        assert lib.ecl_hip_open(C.byref(h), 0, capi.TR | other, 0) == -1, other  # ECL_E_ARG: searched alone, no endomorphism; 8 and 32 unknown
    h = C.c_void_p()
    assert lib.ecl_hip_open(C.byref(h), 0, capi.TR, 0) == 0
    lib.ecl_hip_close(h)
    with pytest.raises(ValueError):
        Device(0, tr=True)  # a33 defaults to True: any other type beside Taproot raises before the library is asked


@pytest.mark.parametrize("start,nkeys,offs", RANGES, ids=["contiguous", "stride128"])
def test_every_key_once_with_the_right_output_key(start, nkeys, offs):
    """all-ones filter: exactly one record per key, type 4, h160 = the leading 20 bytes of the yardstick's output key; both coverage
    totals of the call grow by its keys"""
    d = tr_device(offs=offs)
    try:
        before = d.coverage()
        recs, n = d.add_range(start, nkeys, cap=nkeys + 16)
        grown = tuple(b - a for a, b in zip(before, d.coverage()))
    finally:
        d.close()
    assert n == len(recs) == nkeys and sorted(int(r["key_offset"]) for r in recs) == list(range(nkeys))
    assert all(int(r["compressed"]) == 4 and int(r["endo"]) == 0 for r in recs)
    assert grown == (nkeys, nkeys, nkeys)
    for r in recs:
        k = (start + (int(r["key_offset"]) << offs)) % orc.N
        assert tuple(int(v) for v in r["h160"]) == h160_of(k), int(r["key_offset"])


SLAB_SCRIPT = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from synth import synth_bloom_words
from ecloop_amd import Device
A, n, plant = int(sys.argv[1]), int(sys.argv[2]), json.loads(sys.argv[3])
words = synth_bloom_words(1 << 16, 11, "a|(b&c)")
d = Device(0, a33=False, tr=True)
d.set_bloom(words); d.set_lookahead(0)
d.bloom_insert(np.array(plant, np.uint32))
out = []
for part in json.loads(sys.argv[4]):
    recs, total = d.add_range(A + part[0], part[1], cap=1 << 16)
    assert total == len(recs)
    out += [[part[0] + int(r["key_offset"]), int(r["compressed"]), [int(v) for v in r["h160"]]] for r in recs]
print("COV", json.dumps(d.coverage()))
d.close()
print("RECS", json.dumps(sorted(out)))
""" % (ROOT, os.path.join(ROOT, "tests"))


def slab_run(A, n, plant, parts, slab_log2=None):
    import json
    env = dict(os.environ)
    env.pop("ECL_HIP_TR_SLAB_LOG2", None)
    if slab_log2 is not None:
        env["ECL_HIP_TR_SLAB_LOG2"] = str(slab_log2)
    pr = subprocess.run([sys.executable, "-c", SLAB_SCRIPT, str(A), str(n), json.dumps(plant), json.dumps(parts)], capture_output=True, text=True,
                        timeout=600, env=env)
    assert pr.returncode == 0, pr.stderr[-3000:]
    lines = {l.split(" ", 1)[0]: json.loads(l.split(" ", 1)[1]) for l in pr.stdout.splitlines() if l.startswith(("COV ", "RECS "))}
    return [(r[0], r[1], tuple(r[2])) for r in lines["RECS"]], lines["COV"]


def test_slabs_change_no_record():
    """one call of 3 * 2^20 + 12345 keys under a slab of 2^20 keys, through a filter of bit density 0.625 (0.625^20 = 8e-5 per key: about
    260 chance hits) that also holds the keys at the last offset of each slab, the first of the next and the call's last: the record set
    is identical to the same call under the default slab; every planted key is there; EVERY record, chance hits included, is the
    yardstick's; and the same range as three contiguous calls gives the same records"""
    A, S = 0x5_0000_0000, 1 << 20
    n = 3 * S + 12345
    planted = [S - 1, S, 2 * S - 1, 2 * S, 3 * S - 1, 3 * S, n - 1]
    plant = [list(h160_of(A + off)) for off in planted]
    small, cov = slab_run(A, n, plant, [[0, n]], slab_log2=20)
    default, _ = slab_run(A, n, plant, [[0, n]])
    assert cov == [n, n, n]
    assert small == default and len({r[0] for r in small}) == len(small)
    assert set(planted) <= {r[0] for r in small}
    assert 100 < len(small) < 600, len(small)  # the chance hits were there to be checked
    for off, typ, h in small:
        assert typ == 4 and h == h160_of(A + off), off
    three, cov3 = slab_run(A, n, plant, [[0, S + 77], [S + 77, S], [2 * S + 77, n - 2 * S - 77]], slab_log2=20)
    assert three == small and cov3 == [n, n, n]


def test_overflow_delivers_the_first_records_and_fetch_the_rest():
    import json
    script = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from ecloop_amd import Device
d = Device(0, a33=False, tr=True)
d.set_bloom(np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)); d.set_lookahead(0)
recs, total = d.add_range(0x3F000, 5000, cap=100)
rest = d.fetch_found(100, 4900)
offs = sorted([int(r["key_offset"]) for r in recs] + [int(r["key_offset"]) for r in rest])
assert total == 5000 and len(recs) == 100 and len(rest) == 4900 and offs == list(range(5000)), (total, len(recs), len(rest))
assert all(int(r["compressed"]) == 4 for r in rest)
print("PICK", [[int(r["key_offset"]), [int(v) for v in r["h160"]]] for r in list(recs[:5]) + list(rest[-5:])])
d.close()
""" % ROOT
    pr = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600, env=dict(os.environ, ECL_HIP_TR_SLAB_LOG2="12"))
    assert pr.returncode == 0, pr.stderr[-3000:]
    pick = json.loads([l for l in pr.stdout.splitlines() if l.startswith("PICK ")][0][5:])
    for off, h in pick:
        assert tuple(h) == h160_of(0x3F000 + off)


def test_list_mode_reports_exactly_the_listed_keys():
    start, nkeys = RANGES[0][0], RANGES[0][1]
    listed = sorted(random.Random(5).sample(range(nkeys), 50))
    hs = np.array(sorted(h160_of(start + off) for off in listed), np.uint32)
    d = tr_device()
    try:
        d.set_list(hs)
        recs, n = d.add_range(start, nkeys, cap=4096)
    finally:
        d.close()
    assert n == len(recs) == 50 and sorted(int(r["key_offset"]) for r in recs) == listed
    assert all(tuple(int(v) for v in r["h160"]) == h160_of(start + int(r["key_offset"])) for r in recs)


def test_mul_batch_and_mul_batch_raw_against_the_yardstick():
    """2^16 + 77 seeded random scalars plus 0, n, n - 1, 1 (pageable and page-locked input) and pass phrases of 1 ... 70 bytes, all-ones
    filter: one record per scalar that is not 0 (mod n), each the yardstick's; coverage counts every scalar"""
    from ecloop_amd import capi
    rnd = random.Random(350)
    ks = [rnd.getrandbits(256) for _ in range((1 << 16) + 77)] + [0, orc.N, orc.N - 1, 1]
    want = sorted((i, h160_of(k % orc.N)) for i, k in enumerate(ks) if k % orc.N)
    d = tr_device()
    try:
        cov = d.coverage()
        recs, total = d.mul_batch(ks, cap=len(ks) + 16)
        assert total == len(recs) == len(want) and all(int(r["compressed"]) == 4 for r in recs)
        assert sorted((int(r["key_offset"]), tuple(int(v) for v in r["h160"])) for r in recs) == want
        now = d.coverage()
        assert tuple(b - a for a, b in zip(cov, now)) == (len(ks), len(ks), len(ks))
        K = capi.limbs_array(ks)
        ptr = d.lib.ecl_hip_alloc_host(K.nbytes)  # page-locked by the runtime: the DMA path (the array is above 1 MB)
        assert ptr and K.nbytes >= 1 << 20
        try:
            np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=K.shape)[:] = K
            out = np.zeros(len(ks) + 16, dtype=capi.FOUND_DTYPE)
            cnt = C.c_uint32()
            assert d.lib.ecl_hip_mul_batch(d.h, ptr, len(ks), out.ctypes.data, len(out), C.byref(cnt)) == 0 and cnt.value == len(want)
            assert sorted((int(r["key_offset"]), tuple(int(v) for v in r["h160"])) for r in out[: cnt.value]) == want
        finally:
            d.lib.ecl_hip_free_host(ptr)
        phrases = [bytes(rnd.randrange(32, 127) for _ in range(1 + i % 70)) for i in range(3000)]
        recs, total = d.mul_batch_raw(phrases, cap=4096)
        sc = [int.from_bytes(hashlib.sha256(p).digest(), "big") for p in phrases]
        assert total == len(recs) == len(phrases)
        assert sorted((int(r["key_offset"]), tuple(int(v) for v in r["h160"])) for r in recs) == sorted((i, h160_of(k % orc.N)) for i, k in enumerate(sc))
    finally:
        d.close()


def test_drop_round_fails_add_and_mul_and_the_next_call_is_clean():
    """one provoked COUNT mismatch each (only a loop bound of stage A shrinks): the call returns ECL_E_COVERAGE, the next one is whole"""
    from ecloop_amd import EclError
    d = tr_device(synth_bloom_words(4099, 3, "a|b"))
    try:
        d.set_geometry(8, 256)
        n, A = 1 << 17, 0x7_0000_0000
        good, _ = d.add_range(A, n)
        cov = d.coverage()
        d.diag_drop_round()
        with pytest.raises(EclError) as e:
            d.add_range(A, n)
        assert e.value.code == -8 and len(d.fetch_found(0, 16)) == 0
        now = d.coverage()
        assert now[0] - cov[0] == n and now[1] == cov[1] and now[2] - cov[2] < n
        recs, total = d.add_range(A, n)
        assert total == len(recs) and rec_set(recs) == rec_set(good) and len(recs) > 100
        after = d.coverage()
        assert after[0] - now[0] == after[1] - now[1] == after[2] - now[2] == n
        ks = [0xC0FFEE + 104729 * i for i in range(1000)]
        good, _ = d.mul_batch(ks)
        cov = d.coverage()
        d.diag_drop_round()
        with pytest.raises(EclError) as e:
            d.mul_batch(ks)
        assert e.value.code == -8
        now = d.coverage()
        assert now[0] - cov[0] == 1000 and now[1] == cov[1] and now[2] - cov[2] < 1000
        recs, total = d.mul_batch(ks)
        assert total == len(recs) and rec_set(recs) == rec_set(good)
        for r in recs:
            assert tuple(int(v) for v in r["h160"]) == h160_of(ks[int(r["key_offset"])])
    finally:
        d.close()


def test_lookahead_serves_taproot_jobs_and_keeps_other_types_apart():
    """64 contiguous 2^21-key jobs on a Taproot context: calls are answered from sweeps and the records equal those of the same jobs with
    the look-ahead off; a `-a c` context on the same filter bits is never answered from the Taproot sweeps"""
    from ecloop_amd import Device
    words = synth_bloom_words(4099, 3, "a|b")  # passes one hash in ~300
    A, job, jobs = 0x300000000, 1 << 21, 64
    on, off = tr_device(words, lookahead=1 << 26), tr_device(words)
    c, cplain = Device(0), Device(0)
    try:
        for x, la in ((c, 1 << 26), (cplain, 0)):
            x.set_bloom(words)
            x.set_lookahead(la)
        cmine = []
        on.set_scan_end(A + jobs * job)
        mine, plain = [], []
        for j in range(jobs):
            recs, n = on.add_range(A + j * job, job, cap=1 << 15)
            assert n == len(recs)
            mine += rec_set(recs, A + j * job)
            if 20 <= j < 28:  # the other type walks the same jobs, inside what the Taproot sweeps hold: its records stay its own
                crecs, cn = c.add_range(A + j * job, job, cap=1 << 15)
                assert cn == len(crecs)
                cmine += rec_set(crecs, A + j * job)
        crecs, cn = cplain.add_range(A + 20 * job, 8 * job, cap=1 << 18)
        assert cn == len(crecs) and sorted(cmine) == rec_set(crecs, A + 20 * job) and cmine and all(x[2] == 1 for x in cmine)
        for j in range(jobs):
            recs, n = off.add_range(A + j * job, job, cap=1 << 15)
            plain += rec_set(recs, A + j * job)
        sweeps, _, served, _ = on.lookahead_stats()
        assert sweeps >= 1 and served > 0, (sweeps, served)
        assert sorted(mine) == sorted(plain) and len(mine) > 100000 and all(x[2] == 4 for x in mine)
        for k, _, _, h in mine[:24]:
            assert h == h160_of(k)
        cov = on.coverage()
        assert cov[0] == cov[1] == jobs * job
    finally:
        on.close(), off.close(), c.close(), cplain.close()


def line_of(k):
    return "p2tr: %064x <- %064x" % (tr_ref.output_key(k), k)


def test_cli_add_and_rnd_print_the_whole_output_key(cli, tmp_path):
    keys = (0xdc2a04, 0xffffff, 0x900001)
    lst = tmp_path / "tr.txt"
    lst.write_text("".join("%064x\n" % tr_ref.output_key(k) for k in keys))
    want = sorted(line_of(k) for k in keys)
    r = run_cli(cli, ["add", "-f", str(lst), "-a", "t", "-r", "800000:ffffff"])
    assert r.found == want and counts(r.status) == (3, 8388608), (r.stdout, r.status)
    assert "~ endo: 0 ~ p2tr: 1 | filter: list (3)" in r.stdout
    c = run_cli(cli, ["add", "-f", os.path.join(GOLD, "btc-puzzles-hash"), "-a", "c", "-r", "800000:ffffff"])
    assert counts(c.status)[1] == counts(r.status)[1]  # status-line totals as for -a c on the same range
    blf = str(tmp_path / "tr.blf")
    subprocess.run([cli, "blf-gen", "-a", "t", "-n", "1000", "-o", blf], stdin=open(str(lst), "rb"), stdout=subprocess.PIPE, check=True, timeout=120)
    r = run_cli(cli, ["add", "-f", blf, "-a", "t", "-r", "800000:ffffff"], env={"ECL_HIP_TR_SLAB_LOG2": "20"})
    assert "filter: bloom" in r.stdout and r.found == want and counts(r.status) == (3, 8388608)
    one = tmp_path / "dc.txt"
    one.write_text("%064x\n" % tr_ref.output_key(0xdc2a04))
    r = run_cli(cli, ["rnd", "-f", str(one), "-a", "t", "-seed", "taproot", "-r", "800000:ffffff", "-d", "0:23"])
    assert r.found == [line_of(0xdc2a04)], r.stdout


def test_cli_mul_and_mul_raw_report_the_planted_keys(cli, tmp_path):
    lines = [l.strip() for l in open(os.path.join(GOLD, "mul_scalars.txt")) if l.strip()]
    picked = [orc.sn_from_hex(lines[i]) for i in (3, 77, 200)]
    phrases = [b"taproot test phrase", b"correct horse battery staple", b"key path only"]
    others = [b"phrase %d" % i for i in range(2000)]
    pks = [int.from_bytes(hashlib.sha256(p).digest(), "big") for p in phrases]
    lst = tmp_path / "planted.txt"
    lst.write_text("".join("%064x\n" % tr_ref.output_key(k % orc.N) for k in picked + pks))
    r = run_cli(cli, ["mul", "-f", str(lst), "-a", "t"], stdin_path=os.path.join(GOLD, "mul_scalars.txt"))
    assert r.found == sorted(line_of(k) for k in picked), r.stdout
    assert "~ p2tr: 1 |" in r.stdout
    ph = tmp_path / "phrases.txt"
    ph.write_bytes(b"\n".join(others[:1000] + phrases + others[1000:]) + b"\n")
    r = run_cli(cli, ["mul", "-raw", "-f", str(lst), "-a", "t"], stdin_path=str(ph))
    assert r.found == sorted("p2tr: %064x <- %064x" % (tr_ref.output_key(k % orc.N), k) for k in pks), r.stdout
