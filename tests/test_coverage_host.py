"""Key coverage without a GPU: the C ABI's new return code ECL_E_COVERAGE (-8) in the header, its own strerror text, the two new exports
(ecl_hip_get_coverage, ecl_hip_diag_drop_round) in the built library and in capi, the Python error carrying the code; and, as a guard,
the hidden `plan` command of the host program printing what it printed before the check existed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ecloop_hip.h")
NEW = ("ecl_hip_get_coverage", "ecl_hip_diag_drop_round")


@pytest.fixture(scope="module")
def lib():
    from ecloop_amd.build import build_library
    from ecloop_amd import capi
    build_library()  # no-op when current
    return capi.load()


def test_header_defines_the_coverage_code():
    src = open(HEADER).read()
    m = re.search(r"#define\s+ECL_E_COVERAGE\s+\((-?\d+)\)", src)
    assert m and int(m.group(1)) == -8
    # documented where a binding of the reference's call sites looks: section 1, the seam
    seam = src[src.index("==== 1. THE SEAM"):src.index("==== 2. OPTIONAL")]
    assert "ECL_E_COVERAGE" in seam
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name


def test_strerror_has_its_own_text(lib):
    texts = {rc: lib.ecl_hip_strerror(rc).decode() for rc in range(-8, 1)}
    assert texts[-8] != "unknown error" and texts[-8] not in [t for rc, t in texts.items() if rc != -8]
    assert lib.ecl_hip_strerror(-9).decode() == "unknown error"


def test_library_exports_the_new_calls(lib):
    from ecloop_amd import capi
    for name in NEW:
        assert name in capi.EXPORTS
        getattr(lib, name)  # AttributeError if the symbol is not exported
    assert capi.E_COVERAGE == -8
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    exported = set(re.findall(r"\bT\s+(ecl_hip_\w+)", nm))
    assert set(NEW) <= exported and exported == set(capi.EXPORTS)
    # the header's own count of its exports
    assert "exactly the %d ecl_hip_* functions" % len(capi.EXPORTS) in open(HEADER).read()


def test_null_context_is_refused(lib):
    lib.ecl_hip_get_coverage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ecl_hip_diag_drop_round.argtypes = [C.c_void_p]
    assert lib.ecl_hip_get_coverage(None, None, None, None) == -1
    assert lib.ecl_hip_diag_drop_round(None) == -1


def test_error_carries_the_code():
    from ecloop_amd import EclError
    e = EclError("the device did not hash every key of the call: ...", -8)
    assert e.code == -8 and "every key" in str(e)
    assert EclError("no code").code is None


# what the parent build printed for these ranges: the job arithmetic of add / rnd is untouched by the check
PLAN = {
    ("-r", "8000:ffffff"):
        "stride_bits 0 ord_offs 0 ord_size 24 hashed 0000000000000000000000000000000000000000000000000000000001000000 status_total 16777216 "
        "chunk 4294967296",
    ("-r", "8000:fffff", "-a", "cu", "-endo"):
        "stride_bits 0 ord_offs 0 ord_size 20 hashed 00000000000000000000000000000000000000000000000000000000000f8000 status_total 6094842 "
        "chunk 4294967296",
    ("-r", "20000000000:3ffffffffff", "-d", "64:32"):
        "stride_bits 10 ord_offs 10 ord_size 32 hashed 0000000000000000000000000000000000000000000000000000000080000000 status_total "
        "2147483648 chunk 4294967296",
    ("-r", "8000:ffff", "-t", "3"):
        "stride_bits 0 ord_offs 0 ord_size 20 hashed 0000000000000000000000000000000000000000000000000000000000008000 status_total 32767 "
        "chunk 12288",
}


@pytest.mark.parametrize("args", list(PLAN))
def test_plan_output_is_unchanged(args):
    from ecloop_amd.build import build_host_cli
    cli = build_host_cli()
    out = subprocess.run([cli, "plan"] + list(args), stdout=subprocess.PIPE, check=True, timeout=60).stdout.decode()
    assert out.strip() == PLAN[args]
