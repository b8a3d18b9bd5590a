"""How engine.py's commands collect the hit records of a device call (the caller's half of the overflow protocol of include/ecloop_hip.h:
a call that reports more records than its buffer holds has kept some on the device; they are fetched, and only a short fetch repeats the
call with a buffer that fits) and how KeySearch verifies them, label by label.  The device is a scripted stand-in: it answers from a list
of prepared responses and logs its calls.  Public entry points only."""
import numpy as np
import pytest

from ecloop_amd import capi, engine

GX, GY = engine._G
CODE = {label: code for code, label in capi.LABELS.items()}


def records(n, label="addr33", keys=1, endo=0):
    """n records of one call over `keys` keys: distinct h160 words, key_offset cycling through the keys"""
    a = np.zeros(n, dtype=capi.FOUND_DTYPE)
    for i in range(n):
        a[i]["key_offset"], a[i]["h160"], a[i]["endo"], a[i]["compressed"] = i % keys, [0x1000 * (i + 1) + j for j in range(5)], endo, CODE[label]
    return a


def scripted(script, keep_min=1 << 20, words=None):
    """-> a device class.  script: what each search call produces, in order of the calls (an array of records per call); a call with
    buffer `cap` returns (the first cap records, the total) and keeps max(cap, keep_min) of them for fetch_found, as the library does.
    words: label -> the words the verify methods re-derive (for every key), ok: the flag they return"""

    class Scripted:
        ok = 1

        def __init__(self, device=0, **kw):
            self.kw, self.calls, self.fetches, self.left, self.closed = kw, [], [], list(script), False

        def _call(self, name, cap, **detail):
            self.calls.append(dict(detail, name=name, cap=cap))
            produced = self.left.pop(0)
            self.kept = produced[: max(cap, keep_min)]
            return produced[:cap].copy(), len(produced)

        def mul_batch(self, scalars, cap=4096):
            return self._call("mul_batch", cap, n=len(scalars))

        def mul_batch_raw(self, lines, cap=4096):
            return self._call("mul_batch_raw", cap, n=len(lines))

        def seed_batch(self, phrases, path, passphrase=b"", reuse=False, cap=4096):
            return self._call("seed_batch", cap, n=len(phrases), path=list(path), reuse=reuse)

        def add_range(self, start, nkeys, cap=4096, **kw):
            return self._call("add_range", cap, n=nkeys, **kw)

        def fetch_found(self, first, n):
            self.fetches.append((first, n))
            return self.kept[first : first + n].copy()

        def _ok(self, ks):
            return np.full(len(ks), self.ok, np.uint8)

        def _rows(self, label, ks):
            return np.array([words[label]] * len(ks), dtype=np.uint32)

        def verify(self, ks, origin=None):
            self.calls.append(dict(name="verify", ks=list(ks), origin=origin))
            return self._rows("addr33", ks), self._rows("addr65", ks), self._ok(ks)

        def p2sh_hash(self, h33):
            assert [list(map(int, h)) for h in h33] == [words["addr33"]] * len(h33)
            return self._rows("p2sh", h33)

        def verify_eth(self, ks, origin=None):
            self.calls.append(dict(name="verify_eth", ks=list(ks), origin=origin))
            return self._rows("eth", ks), self._ok(ks)

        def verify_tr(self, ks):
            return self._rows("p2tr", ks), self._ok(ks)

        def verify_pub(self, ks):
            return self._rows("pub", ks), np.ones(len(ks), np.uint8), self._ok(ks)

        def geometry(self):
            return 64, 512

        def set_bloom(self, words):
            pass

        set_prefixes = set_list = set_bloom

        def get_bloom(self, nwords):
            return np.zeros(nwords, np.uint64)

        def close(self):
            self.closed = True

    return Scripted


ANY = engine.Filter(np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64))  # bloom mode: every record is confirmed
PATH = "m/0'"


def run_mul(dev_cls):
    ks = engine.KeySearch(ANY, device_cls=dev_cls, verify=False)
    scalars = [5, 6, 7, 8]
    ks.cmd_mul(scalars, cap=8)
    return ks, 4, [scalars[i % 4] for i in range(12)]


def run_mul_raw(dev_cls):
    ks = engine.KeySearch(ANY, device_cls=dev_cls, verify=False)
    lines = [b"a", b"b", b"c", b"d"]
    ks.cmd_mul_raw(lines, cap=8)
    return ks, 4, [int.from_bytes(engine.kdf_digest("sha256", lines[i % 4]), "big") for i in range(12)]


def run_seed(dev_cls):
    ks = engine.KeySearch(ANY, device_cls=dev_cls, verify=False, bip39=True)
    phrases = [b"w", b"x", b"y", b"z"]
    ks.cmd_seed(phrases, [PATH], cap=8)
    assert all(r.path == PATH and r.phrase == phrases[i % 4] for i, r in enumerate(ks.found))
    return ks, 4, [engine.bip39_key(phrases[i % 4], PATH) for i in range(12)]


COMMANDS = {"cmd_mul": (run_mul, "mul_batch"), "cmd_mul_raw": (run_mul_raw, "mul_batch_raw"), "cmd_seed": (run_seed, "seed_batch")}


def check(ks, produced, checked, keys):
    """every record of the call found once, in the call's order, with the key of its line; the counters"""
    assert [r.h160 for r in ks.found] == [[int(w) for w in p["h160"]] for p in produced]
    assert [r.pk for r in ks.found] == keys[: len(produced)] and [r.label for r in ks.found] == ["addr33"] * len(produced)
    assert (ks.k_found, ks.k_checked) == (len(produced), checked)


@pytest.mark.parametrize("cmd", sorted(COMMANDS))
def test_records_that_fit_take_one_call_and_no_fetch(cmd):
    run, name = COMMANDS[cmd]
    produced = records(8, keys=4)  # cap = max(8, 2 * 4) = 8
    ks, checked, keys = run(scripted([produced]))
    check(ks, produced, checked, keys)
    assert [(c["name"], c["cap"]) for c in ks.dev.calls] == [(name, 8)] and ks.dev.fetches == []


@pytest.mark.parametrize("cmd", sorted(COMMANDS))
def test_overflow_the_device_kept_is_fetched_once(cmd):
    run, name = COMMANDS[cmd]
    produced = records(12, keys=4)
    ks, checked, keys = run(scripted([produced]))
    check(ks, produced, checked, keys)
    assert [(c["name"], c["cap"]) for c in ks.dev.calls] == [(name, 8)] and ks.dev.fetches == [(8, 4)]


@pytest.mark.parametrize("cmd", sorted(COMMANDS))
def test_a_short_fetch_repeats_the_call_with_a_buffer_that_fits(cmd):
    run, name = COMMANDS[cmd]
    produced = records(12, keys=4)
    ks, checked, keys = run(scripted([produced, produced], keep_min=10))
    check(ks, produced, checked, keys)
    assert [(c["name"], c["cap"]) for c in ks.dev.calls] == [(name, 8), (name, 12)] and ks.dev.fetches == [(8, 4)]


def test_cmd_seed_repeats_a_reuse_call_as_a_reuse_call():
    """two paths: the second is a reuse call, and its repeat after a short fetch is one too"""
    first, second = records(4, keys=4), records(12, keys=4)
    ks = engine.KeySearch(ANY, device_cls=scripted([first, second, second], keep_min=10), verify=False, bip39=True)
    ks.cmd_seed([b"w", b"x", b"y", b"z"], ["m/0'", "m/1'"], cap=8)
    assert [(c["reuse"], c["cap"], c["path"]) for c in ks.dev.calls] == [(False, 8, [1 << 31]), (True, 8, [1 << 31 | 1]), (True, 12, [1 << 31 | 1])]
    assert (ks.k_found, ks.k_checked) == (16, 8) and [r.path for r in ks.found] == ["m/0'"] * 4 + ["m/1'"] * 12


def test_add_keys_passes_no_origin_keyword_without_an_origin():
    produced = records(12, keys=2048)
    ks = engine.KeySearch(ANY, device_cls=scripted([produced, produced], keep_min=10), verify=False)
    ks.add_keys(0x8000, 2048, cap=8)
    assert ks.dev.kw == dict(a33=True, a65=False, endo=False, ord_offs=0)  # flags reach the device class only when set
    assert ks.dev.calls == [dict(name="add_range", cap=8, n=2048), dict(name="add_range", cap=12, n=2048)] and ks.dev.fetches == [(8, 4)]
    assert [r.pk for r in ks.found] == [0x8000 + i for i in range(12)] and ks.k_found == 12


def test_kangaroo_round_with_more_records_than_the_device_keeps_raises():
    made = []

    def dev_cls(*a, **kw):
        made.append(scripted([records(4100 + 8, label="dp")], keep_min=0)(*a, **kw))
        return made[0]

    with pytest.raises(engine.EclError, match="^kangaroo: more records in one round than the device keeps; use more dp bits$"):
        engine.kangaroo_search((GX, GY), 1, 1 << 20, herd_log2=1, dp_bits=0, round_steps=1, device_cls=dev_cls)
    d = made[0]
    assert [(c["name"], c["cap"], c["n"]) for c in d.calls] == [("add_range", 4100, 2)] and d.fetches == [(4100, 8)] and d.closed


def test_bsgs_call_with_more_records_than_the_device_keeps_raises():
    made = []

    def dev_cls(*a, **kw):
        script = [records(0)] if kw.get("insert") else [records(12, label="pub")]
        made.append(scripted(script, keep_min=0)(*a, **kw))
        return made[-1]

    with pytest.raises(engine.EclError, match="^bsgs: more records in one call than the device keeps; use a larger filter$"):
        engine.bsgs_search((GX, GY), 1, 1 << 16, baby_log2=4, device_cls=dev_cls, cap=8)
    giant = made[1]
    assert [c["cap"] for c in giant.calls] == [8] and giant.fetches == [(8, 4)] and giant.closed


# ---- KeySearch's verification of the records (pk_verify_hash), label by label, through add_keys

WORDS = {"addr33": [11, 12, 13, 14, 15], "addr65": [21, 22, 23, 24, 25], "p2sh": [31, 32, 33, 34, 35], "eth": [41, 42, 43, 44, 45],
         "p2tr": [51, 52, 53, 54, 55, 56, 57, 58], "pub": [61, 62, 63, 64, 65, 66, 67, 68]}
FLAGS = {"addr33": {}, "addr65": {"a33": False, "a65": True}, "p2sh": {"a33": False, "p2sh": True}, "eth": {"eth": True}, "p2tr": {"tr": True},
         "pub": {"pub": True}}
SPLIT = {"addr65": {"a33": False, "a65": True}, "eth": {"eth": True}}  # split-key records: the labels whose words come from another place
CASES = [(label, False) for label in sorted(WORDS)] + [(label, True) for label in sorted(SPLIT)]


def key_of(split):
    return engine.calc_priv(0x8000, 1, 0, 3 if split else 0)  # (a split-key record's key is the partial key of its image)


def verified(label, split, flip=None, ok=1):
    rec = records(1, label=label, keys=2048, endo=3 if split else 0)
    rec[0]["h160"] = WORDS[label][:5]
    if flip is not None:
        rec[0]["h160"][flip] ^= 1
    dev_cls = scripted([rec], words=WORDS)
    dev_cls.ok = ok
    if split:
        ks = engine.KeySearch(engine.PrefixFilter(np.zeros((1, 10), np.uint32)), device_cls=dev_cls, prefix=True, origin=(GX, GY), **SPLIT[label])
    else:
        ks = engine.KeySearch(ANY, device_cls=dev_cls, **FLAGS[label])
    ks.add_keys(0x8000, 2048)
    return ks


@pytest.mark.parametrize("label,split", CASES)
def test_a_record_with_the_rederived_words_passes(label, split):
    ks = verified(label, split)
    (r,) = ks.found
    assert (r.label, r.pk, ks.k_found) == (label, key_of(split), 1)
    assert r.h160 == (WORDS[label] if label in ("p2tr", "pub") else WORDS[label][:5])  # p2tr / pub: all eight words of the key
    assert r.prefix == ("03" if label == "pub" else "")
    if split:  # the partial key, re-derived from the same image of the origin: endo 3 = x times beta, y negated
        image = (GX * engine.SPLITKEY_BETA % engine.P, engine.P - GY)
        assert r.split == 3 and ks.dev.calls[-1] == dict(name="verify_eth" if label == "eth" else "verify", ks=[key_of(split)], origin=[image])
        assert ks.dev.calls[0] == dict(name="add_range", cap=4096, n=2048, origin=(GX, GY))


@pytest.mark.parametrize("word", [0, 4])
@pytest.mark.parametrize("label,split", CASES)
def test_a_record_with_one_word_flipped_is_a_hash_mismatch(label, split, word):
    with pytest.raises(engine.EclError, match=r"^\[!\] error: hash mismatch \(%s\) pk: %064x$" % (label, key_of(split))):
        verified(label, split, flip=word)


@pytest.mark.parametrize("label,split", CASES)
def test_a_record_whose_key_the_device_could_not_rederive_is_a_hash_mismatch(label, split):
    with pytest.raises(engine.EclError, match=r"hash mismatch \(%s\)" % label):
        verified(label, split, ok=0)
