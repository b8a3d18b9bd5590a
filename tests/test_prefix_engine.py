"""engine.prefix_search on a stand-in device (no GPU): the oracle hashes the keys, a Python range test stands for the device's prefix
filter, and the yardstick tests/prefix_ref.py says which addresses start with the patterns."""
import numpy as np
import pytest

import orc
import prefix_ref as R
from fake_device import FakeDevice
from ecloop_amd import capi, engine


class FakePrefixDevice(FakeDevice):
    """FakeDevice with the prefix surface: set_prefixes takes the table, add_range reports the records whose value lies inside a range"""
    tables = []
    report_everything = False  # a device whose filter lets every hash through: the host's text comparison has to drop them

    def __init__(self, device=0, a33=True, a65=False, endo=False, ord_offs=0, prefix=False):
        assert prefix
        super().__init__(device, a33=a33, a65=a65, endo=endo, ord_offs=ord_offs)
        self.words = np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64)
        self.pairs = None

    def set_bloom(self, words):
        raise AssertionError("a prefix search sets a table, not a bloom filter")

    def set_prefixes(self, table):
        table = np.asarray(table)
        assert table.dtype == np.uint32 and table.ndim == 2 and table.shape[1] == 10
        FakePrefixDevice.tables.append(table.copy())
        self.pairs = [(R.value_of(r[:5]), R.value_of(r[5:])) for r in table]

    def add_range(self, start, nkeys, cap=4096):
        everything, _ = super().add_range(start, nkeys, cap=1 << 20)
        keep = [i for i, r in enumerate(everything) if self.report_everything or R.in_table(self.pairs, R.value_of(r["h160"]))]
        arr = everything[keep]
        self.kept = arr
        return arr[:cap].copy(), len(arr)


def all_records(start, nkeys, a33, a65, endo):
    d = FakeDevice(0, a33=a33, a65=a65, endo=endo)
    d.set_bloom(np.full(64, 0xFFFFFFFFFFFFFFFF, np.uint64))
    recs, n = d.add_range(start, nkeys, cap=1 << 20)
    assert n == len(recs)
    return recs


@pytest.mark.parametrize("a33,a65,endo", [(True, False, False), (True, True, True)], ids=["c", "cu-endo"])
def test_prefix_search_reports_the_matching_keys_with_their_addresses(a33, a65, endo):
    start, nkeys = 0x8000, 4096
    recs = all_records(start, nkeys, a33, a65, endo)
    # patterns from addresses that are there: five characters of two keys' addresses (about 2^-23 each), and a bc1q form when -a c alone
    v1, v2 = R.value_of(recs[100]["h160"]), R.value_of(recs[len(recs) // 2]["h160"])
    patterns = [R.p2pkh(v1)[:5], R.p2pkh(v2)[:5]] + ([R.p2wpkh(v2)[:9]] if not a65 else [])
    label = lambda r: "addr33" if r["compressed"] else "addr65"
    want = {}
    for r in recs:
        v = R.value_of(r["h160"])
        first = next((p for p in patterns if not (p.startswith("bc1q") and not r["compressed"]) and R.matches(p, v)), None)
        if first is not None:
            pk = engine.calc_priv(start, 1, int(r["key_offset"]), int(r["endo"]))
            want[(label(r), v, pk)] = R.address(first, v)
    assert len(want) >= 2
    FakePrefixDevice.tables.clear()
    found, edge = engine.prefix_search(patterns, start, start + nkeys, a33=a33, a65=a65, endo=endo, device_cls=FakePrefixDevice)
    got = {(f.label, R.value_of(f.h160), f.pk): f.address for f in found}
    assert got == want and len(found) == len(want) and edge == 0
    table, _ = engine.prefix_ranges(patterns, a33, a65, False)
    assert len(FakePrefixDevice.tables) == 1 and (FakePrefixDevice.tables[0] == table).all()
    f = found[0]
    assert f.stdout_line() == "%s: %040x <- %064x %s" % (f.label, R.value_of(f.h160), f.pk, f.address)
    assert f.line() == "%s\t%040x\t%064x\t%s" % (f.label, R.value_of(f.h160), f.pk, f.address)


def test_records_whose_text_matches_no_pattern_are_dropped_and_counted(monkeypatch):
    start, nkeys = 0x8000, 2048
    recs = all_records(start, nkeys, True, False, False)
    pattern = R.p2pkh(R.value_of(recs[7]["h160"]))[:6]
    monkeypatch.setattr(FakePrefixDevice, "report_everything", True)
    found, edge = engine.prefix_search([pattern], start, start + nkeys, device_cls=FakePrefixDevice)
    matching = [r for r in recs if R.matches(pattern, R.value_of(r["h160"]))]
    assert len(found) == len(matching) >= 1 and edge == len(recs) - len(matching)
    assert all(f.address.startswith(pattern) for f in found)


def test_refused_patterns_reach_no_device():
    class Never:
        def __init__(self, *a, **k):
            raise AssertionError("opened a device for a refused pattern")
    for patterns, kw in ((["1l"], {}), (["0xdead"], {}), (["1Q"], {}), (["bc1qw508"], {"a65": True}), (["3J98t1"], {}), ([], {})):
        with pytest.raises(engine.PrefixError):
            engine.prefix_search(patterns, 0x8000, 0x9000, device_cls=Never, **kw)
    assert issubclass(engine.PrefixError, ValueError) and capi.PREFIX == 4096
