"""tests/support.py itself, on the CPU: the status-line counters, the stderr / stdout filters of run_cli, and rec_set."""
import json
import os

import numpy as np

import support
from ecloop_amd import capi


def test_counts_reads_the_golden_status_counters():
    """the counters golden.json records, written the way the host program's status line writes them (host/cli_report.h: with and
    without the locale's thousands separators, with the key hint of a line that is still running)"""
    cases = json.load(open(os.path.join(support.GOLD, "golden.json")))["cases"]
    pairs = {(g["status_found"], g["status_checked"]) for g in cases.values() if "status_found" in g} | \
            {tuple(g["status"]) for g in cases.values() if "status" in g}
    assert len(pairs) > 10
    for found, checked in pairs:
        for tail in ("%d / %d" % (found, checked), "{:,} / {:,}".format(found, checked)):
            assert support.counts("3.21s ~ 1234.56 Mkeys/s ~ " + tail) == (found, checked)
            assert support.counts("0.00s ~ 0.00 Mkeys/s ~ " + tail + " ('p' – pause)") == (found, checked)


def test_last_status_line_and_found_lines():
    err = "[i] list: 2 entries\n0.50s ~ 1.00 Mkeys/s ~ 0 / 500,000 ('p' – pause)\r\x1b[2K1.00s ~ 2.00 Mkeys/s ~ 1 / 2,000,000 ('p' – pause)\r" \
          "\x1b[2K1.50s ~ 2.00 Mkeys/s ~ 2 / 3,000,000\n"
    assert support.last_status(err) == "1.50s ~ 2.00 Mkeys/s ~ 2 / 3,000,000"
    assert support.counts(support.last_status(err)) == (2, 3000000)
    assert support.last_status("") == "" and support.last_status("plain\n") == "plain"
    out = "threads: 1 ~ addr33: 1 | filter: list (2)\n----\np2sh: bb <- 02\naddr33: aa <- 01\nnote: no arrow\na <- b\n"
    assert support.found_lines(out) == ["addr33: aa <- 01", "p2sh: bb <- 02"]


def test_rec_set_with_and_without_a_base():
    recs = np.zeros(3, capi.FOUND_DTYPE)
    recs["key_offset"] = [7, 2, 2]
    recs["endo"] = [0, 5, 1]
    recs["compressed"] = [1, 0, 1]
    recs["h160"] = [[1, 2, 3, 4, 5], [9, 9, 9, 9, 9], [0, 0, 0, 0, 1]]
    assert support.rec_set(recs) == [(2, 1, 1, (0, 0, 0, 0, 1)), (2, 5, 0, (9, 9, 9, 9, 9)), (7, 0, 1, (1, 2, 3, 4, 5))]
    assert support.rec_set(recs, base=1 << 70) == [((1 << 70) + k, e, c, h) for k, e, c, h in support.rec_set(recs)]
    assert all(type(v) is int for t in support.rec_set(recs) for v in t[:3]) and support.rec_set(recs[:0]) == []
