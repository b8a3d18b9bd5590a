"""What a search call decides from the counter words it reads back (csrc/callstate.h: call_verdict_of) without a GPU:
csrc/tools/callstate_host.cpp walks a table of cases through the function and compares every output field - records below, at and past
the caller's cap and past what the device keeps, with and without a list (which word counts, where the records start), a list whose
bloom hits outran the staging area, a key count short and long by one, the second count short while the first is whole, cap 0 - and the
texts, the three transitions of the last call's records, the coverage totals by result.  Built as a program of its own with the address
and undefined-behaviour sanitizers and run.  The text checks below keep the counter words and the last records behind their names."""
import os
import re

from support import CSRC, ROOT, host_program, run_program


def code_of(path):
    return re.sub(r"/\*.*?\*/", "", re.sub(r"//.*", "", open(path).read()), flags=re.S)


def host_code():
    names = ["ecloop_hip.hip"] + sorted(n for n in os.listdir(CSRC) if n.startswith("abi_") and n.endswith(".h"))
    assert len(names) >= 7
    return {n: code_of(os.path.join(CSRC, n)) for n in names}


def test_the_verdict_table_holds_under_the_sanitizers(tmp_path):
    pr = run_program(host_program(tmp_path, "callstate_host.cpp", ["-O0", "-Wall", "-Werror"]))
    assert pr.returncode == 0 and pr.stderr == "", (pr.stdout, pr.stderr)
    m = re.search(r"callstate_host: ok \((\d+) cases\)", pr.stdout)
    assert m and int(m.group(1)) >= 14, pr.stdout


def test_the_header_needs_no_hip_and_the_build_stamp_sees_it():
    from ecloop_amd import build
    uses_hip = re.compile(r"<hip/|hip_runtime|\bhip[A-Z]\w*|__global__|__device__")
    for path in (os.path.join(CSRC, "callstate.h"), os.path.join(ROOT, "include", "ecloop_hip.h")):  # (the one header it includes)
        assert not uses_hip.search(code_of(path)), path
    assert re.findall(r'#include\s+"([^"]+)"', code_of(os.path.join(CSRC, "callstate.h"))) == ["../../include/ecloop_hip.h"]
    assert "callstate.h" in build.SOURCES


def test_counter_words_go_by_their_names():
    """no host code indexes the counters (or their page-locked copy) with a number"""
    literal = re.compile(r"\b(d_counter|pin_counter)\.p\s*(\[\s*\d|\+\s*\d)|\bECL_COUNTER_WORDS\b")
    for name, text in host_code().items():
        assert not literal.search(text), (name, literal.search(text).group(0))
    assert "CW_KEYS" in host_code()["ecloop_hip.hip"]  # (the check reads the files it means to)


def test_the_last_records_change_through_their_transitions_only():
    """outside callstate.h no code assigns a member of the context's last_records, and the loose last_* members are gone"""
    members = "at|held|total|endo|from_host|region|host_at|n|off"
    assigns = re.compile(r"\blast\s*\.\s*(%s)\s*(=(?!=)|[-+|&^]=|\+\+|--)|\blast_(%s|host_n|host_off)\b" % (members, members))
    for name, text in host_code().items():
        assert not assigns.search(text), (name, assigns.search(text).group(0))
    used = "".join(host_code().values())
    assert all("last.%s(" % t in used for t in ("forget", "on_device", "on_host"))
