"""The library's owning, growable buffer (csrc/devbuf.h: every device and page-locked buffer of a context) without a GPU:
csrc/tools/devbuf_host.cpp includes the header with a counting stand-in allocator that can fail its k-th allocation and checks the rules the
grow sites rely on - a grow to no more than is held keeps the pointer; a larger one frees once and allocates once; a failed one leaves
the buffer empty and a later one succeeds; move, swap and release() hand the buffer on with no double free; a group of four buffers
whose third allocation fails has the capacity of its smallest member and is completed by the next grow with exactly two allocations;
allocations equal frees at exit.  Built as a program of its own with the address and undefined-behaviour sanitizers and run."""
import os
import re

from support import CSRC, host_program, run_program


def test_the_buffer_rules_hold_under_the_sanitizers(tmp_path):
    pr = run_program(host_program(tmp_path, "devbuf_host.cpp", ["-O0", "-Wall", "-Werror"]))
    assert pr.returncode == 0 and pr.stderr == "", (pr.stdout, pr.stderr)
    m = re.search(r"devbuf_host: ok \((\d+) allocations, (\d+) frees\)", pr.stdout)
    assert m and int(m.group(1)) == int(m.group(2)) > 0, pr.stdout


def test_the_header_needs_no_hip_and_the_build_stamp_sees_it():
    from ecloop_amd import build
    text = open(os.path.join(CSRC, "devbuf.h")).read()
    assert "hip" not in re.sub(r"//.*", "", text).lower()
    assert "devbuf.h" in build.SOURCES


def test_allocation_calls_live_in_the_two_policies_only():
    """the library's host code obtains and returns device / page-locked memory through the two policies of ecloop_hip.hip, and through the
    caller-facing pair ecl_hip_alloc_host / ecl_hip_free_host; ecl_hip_close names no buffer"""
    calls = re.compile(r"\b(hipFree|hipHostFree|hipMalloc|hipHostMalloc)\(")
    main = open(os.path.join(CSRC, "ecloop_hip.hip")).read()
    for name in sorted(os.listdir(CSRC)):
        if name.startswith("abi_") and name.endswith(".h"):
            assert not calls.search(open(os.path.join(CSRC, name)).read()), name

    def body(start, end):
        return main[main.index(start):main.index(end, main.index(start))]
    allowed = body("struct dev_mem {", "template <typename T> using devbuf") + body("void* ecl_hip_alloc_host(", "int ecl_hip_set_list(")
    assert len(calls.findall(main)) == len(calls.findall(allowed)) == 6
    close = body("void ecl_hip_close(", "\n}\n")
    assert "delete h;" in close and not re.search(r"\b(d_|pin_)\w+", close), close
