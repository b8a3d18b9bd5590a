"""What the test files share: paths, host builds of csrc/tools/*_host.cpp (as a shared object for ctypes, or as a stand-alone program
under the sanitizers), the long phrase lengths of the seed tests, the `cli` fixture, one runner for the host program with its status line and found lines picked out, and the
record-to-tuples helper.  A plain module: pytest does not rewrite its asserts, so each one carries its message."""
import ctypes
import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "ecloop_amd", "csrc")
TOOLS_SRC = os.path.join(CSRC, "tools")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# phrase lengths behind the 300 bytes the seed tests began with: the empty phrase; 4 to 9 SHA-512 blocks in steps of 7; around every block
# end up to 8 blocks - 111 / 112 mod 128 is where the padding spills into a block of its own; the host program's piece of 1024; 16 and 32 blocks
SEED_LONG_LENS = list(dict.fromkeys([0] + list(range(261, 1101, 7)) + [128 * b + d for b in range(2, 9) for d in (-17, -16, -1, 0, 1)] + [1023, 1024, 1025, 2000, 4000]))
assert len(SEED_LONG_LENS) == 154


def host_lib(tmp_path_factory, source, extra=()):
    """csrc/tools/<source> compiled for the host as a shared object (g++ -O2; `extra`: further sources or flags), loaded with ctypes"""
    stem = os.path.splitext(source)[0]
    so = str(tmp_path_factory.mktemp(stem) / ("lib%s.so" % stem))
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", *extra, "-o", so, os.path.join(TOOLS_SRC, source)], check=True)
    return ctypes.CDLL(so)


def host_program(tmp_path, source, flags, sanitize=True):
    """csrc/tools/<source> built with its own main as a stand-alone program, under ASan + UBSan with errors fatal unless told otherwise;
    `flags`: the site's optimisation level and warnings.  -> the program's path"""
    exe = os.path.join(str(tmp_path), os.path.splitext(source)[0] + ("_san" if sanitize else ""))
    subprocess.run(["g++", *flags, "-std=c++17", *(SANITIZE if sanitize else []), "-o", exe, os.path.join(TOOLS_SRC, source)], check=True)
    return exe


def run_program(exe, timeout=120):
    return subprocess.run([exe], capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def cli():
    from ecloop_amd.build import build_host_cli, build_library
    build_library()
    return build_host_cli()


def last_status(stderr):
    """the status line as it stood last: the text after the final carriage return or erase-line sequence"""
    return stderr.replace("\x1b[2K", "\r").split("\r")[-1].strip()


def found_lines(stdout):
    return sorted(l for l in stdout.splitlines() if ": " in l and " <- " in l)


def run_cli(cli, args, *, stdin_path=None, stdin=None, out=None, env=None, timeout=600, hard_limit=None, check=True):
    """One run of the host program.  `out`: adds -q -o <out>, whose sorted lines are `lines`; `stdin_path` / `stdin`: a file / a string to
    feed it; `env`: merged over os.environ; `hard_limit`: seconds under `timeout -k 10`; `check`: exit status 0, or the tail of stderr.
    -> returncode, stdout, stderr, status (the last status line), found (the sorted found lines of stdout), lines"""
    cmd = (["timeout", "-k", "10", str(hard_limit)] if hard_limit else []) + [cli] + list(args) + (["-q", "-o", out] if out else [])
    feed = {"input": stdin.encode()} if stdin is not None else {"stdin": open(stdin_path, "rb") if stdin_path else subprocess.DEVNULL}
    pr = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=dict(os.environ, **(env or {})), **feed)
    stdout, stderr = pr.stdout.decode(errors="replace"), pr.stderr.decode(errors="replace")
    if check:
        assert pr.returncode == 0, "exit status %d: %s" % (pr.returncode, stderr[-2000:])
    lines = sorted(l.rstrip("\n") for l in open(out)) if out and os.path.exists(out) else []
    return SimpleNamespace(returncode=pr.returncode, stdout=stdout, stderr=stderr, status=last_status(stderr), found=found_lines(stdout), lines=lines)


def counts(status):
    """(found, checked) of a status line"""
    found, checked = status.split("~")[-1].split("/")
    clean = lambda s: int("".join(c for c in s if c.isdigit()))
    return clean(found), clean(checked)


def rec_set(recs, base=0):
    return sorted((base + int(r["key_offset"]), int(r["endo"]), int(r["compressed"]), tuple(int(v) for v in r["h160"])) for r in recs)


def kept_assembly():
    """the assembly the library's build keeps beside it (built first where hipcc is there); skips where there is neither"""
    from ecloop_amd.build import ASM, build_library
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        build_library()  # no-op when current; always leaves the assembly of the shipped code object beside the library
    if not os.path.exists(ASM):
        pytest.skip("no hipcc and no kept assembly: nothing to analyse")
    return ASM


def int_of(limbs):
    """the integer of little-endian 64-bit limbs"""
    return sum(int(v) << (64 * i) for i, v in enumerate(limbs))


def words8(v):
    """256 bits as eight little-endian 32-bit words"""
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def int_of_words(w):
    """the integer of little-endian 32-bit words"""
    return sum(int(v) << (32 * i) for i, v in enumerate(w))
