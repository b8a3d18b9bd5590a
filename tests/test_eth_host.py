"""Ethereum addresses (-a e, ECL_ETH) without a GPU: the yardstick (tests/eth_ref.py) pinned against hashlib's SHA3-256; eth_address of
the device header keccak.h compiled for the host against it; the C ABI header's flag and entry point; the CLI's help text, its refusal of
mixed type strings and its reading of 0x-prefixed, mixed-case address lists; and, from the assembly the build keeps, the registers and
loops of the three ETH kernels."""
import ctypes as C
import hashlib
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import eth_ref
import orc
from support import ROOT, cli, host_lib, kept_assembly, words8

sys.path.insert(0, os.path.join(ROOT, "tools"))

# private key -> Ethereum address
KNOWN = {1: "7e5f4552091a69125d5dfcb7b8c2659029395bdf", 2: "2b5ad5c4795c026514f8317c7a215e218dccd6cf",
         0xdc2a04: "d2c71c0b28f045d0e6facc19a3a6a81a85a17ce4", 0x8000: "8af7c4e8e5f28db7cd19ad12818458d73547d2ec",
         0xffffff: "1c68cf50fac5639f9fd70946be6c2fcfdff19f33"}


def test_the_yardstick_is_sha3_with_another_pad_byte_and_gives_the_known_addresses():
    rnd = random.Random(1600)
    for n in list(range(0, 301, 3)) + [135, 136, 137, 271, 272, 273]:  # around the rate's multiples too
        msg = bytes(rnd.randrange(256) for _ in range(n))
        assert eth_ref.keccak256(msg, 0x06) == hashlib.sha3_256(msg).digest(), n
    assert eth_ref.self_check()
    for k, want in KNOWN.items():
        assert eth_ref.eth_hex(*orc.point_of(k)) == want, hex(k)


@pytest.fixture(scope="module")
def E(tmp_path_factory):
    lib = host_lib(tmp_path_factory, "eth_host.cpp")
    lib.eh_eth_many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    return lib


def device_eth(E, xs, ys):
    X = np.array([words8(x) for x in xs], np.uint32)
    Y = np.array([words8(y) for y in ys], np.uint32)
    out = np.zeros((len(X), 5), np.uint32)
    E.eh_eth_many(X.ctypes.data, Y.ctypes.data, out.ctypes.data, len(X))
    return out


def test_keccak_h_known_answers(E):
    pts = [orc.point_of(k) for k in KNOWN]
    got = device_eth(E, [p[0] for p in pts], [p[1] for p in pts])
    assert [orc.hex160(g) for g in got] == list(KNOWN.values())


def test_keccak_h_random_words_against_the_yardstick(E):
    rnd = random.Random(256)
    xs = [0, (1 << 256) - 1] + [rnd.getrandbits(256) for _ in range(10000)]  # any words: they need not be curve points
    ys = [0, (1 << 256) - 1] + [rnd.getrandbits(256) for _ in range(10000)]
    got = device_eth(E, xs, ys)
    for i in range(len(xs)):
        assert [int(v) for v in got[i]] == eth_ref.eth_words(xs[i], ys[i]), i


def test_header_declares_the_flag_and_the_entry_point():
    header = open(os.path.join(ROOT, "include", "ecloop_hip.h")).read()
    assert re.search(r"#define ECL_ETH 64u\b", header)  # (8 and 32 stay unknown flags: tests/test_gpu_primitives.py, tests/test_gpu_p2sh.py)
    assert re.search(r"int ecl_hip_verify_eth\(ecl_hip \*h, const uint64_t \(\*k\)\[4\], uint32_t n, uint32_t \(\*addr\)\[5\], uint8_t \*ok\);", header)
    assert "eth is searched alone" in header.lower()
    from ecloop_amd import capi
    assert capi.ETH == 64 and "ecl_hip_verify_eth" in capi.EXPORTS and capi.label_of(3) == "eth"


def test_cli_help_names_the_eth_letter_and_mixed_type_strings_are_refused(cli):
    out = subprocess.run([cli], capture_output=True, text=True, timeout=60).stdout
    line = [l for l in out.splitlines() if l.strip().startswith("-a ")]
    assert len(line) == 1 and re.search(r"\be - eth\b", line[0]) and re.search(r"\bs - p2sh\b", line[0]), out
    for verb in ("add", "mul", "rnd"):
        for mixed in ("ce", "es", "ue"):  # refused before the filter is opened or a GPU is looked for
            pr = subprocess.run([cli, verb, "-a", mixed, "-f", "/nonexistent", "-r", "8000:ffff"], stdin=subprocess.DEVNULL, capture_output=True,
                                text=True, timeout=60)
            assert pr.returncode != 0 and "eth is searched alone" in pr.stderr, (verb, mixed, pr.stderr)


def eip55(addr):
    """EIP-55: hex digit i is upper case when nibble i of Keccak-256(the lower-case hex text) is >= 8"""
    h = eth_ref.keccak256(addr.encode()).hex()
    return "".join(c.upper() if int(h[i], 16) >= 8 else c for i, c in enumerate(addr))


@pytest.mark.parametrize("decoder", ["ssse3", "scalar"])
def test_address_lists_with_0x_and_mixed_case_are_read_with_a_e_only(cli, tmp_path, decoder):
    """blf-gen (host path: a small filter) then blf-check: with -a e every line of the file is an entry - 0x + EIP-55 mixed case, plain
    lower case, 0X + upper case; without -a e only the un-prefixed lines are (the prefixed ones are read as they always were: no entry).
    Both decoders of hash160_from_hex: SSSE3 (where the CPU has it) and the scalar table, which ECLOOP_HIP_NO_SSSE3 selects"""
    env = dict(os.environ, **({"ECLOOP_HIP_NO_SSSE3": "1"} if decoder == "scalar" else {}))
    addrs = list(KNOWN.values())
    assert eip55(addrs[0]) != addrs[0] and eip55(addrs[0]).lower() == addrs[0]
    prefixed = ["0x" + eip55(addrs[0]), "0x" + eip55(addrs[1]), "0X" + addrs[2].upper()]
    plain = [addrs[3], eip55(addrs[4])]
    text = "\n".join(prefixed[:2] + plain[:1] + prefixed[2:] + plain[1:]) + "\n"
    for with_e, want in ((True, set(addrs)), (False, {a.lower() for a in plain})):
        blf = str(tmp_path / ("l%d.blf" % with_e))
        cmd = [cli, "blf-gen", "-n", "1000", "-o", blf] + (["-a", "e"] if with_e else [])
        pr = subprocess.run(cmd, input=text.encode(), capture_output=True, timeout=120, env=env)
        assert pr.returncode == 0, pr.stderr
        assert b"added %d new items" % len(want) in pr.stdout, (with_e, pr.stdout)
        pr = subprocess.run([cli, "blf-check", "-f", blf] + addrs, capture_output=True, text=True, timeout=120, env=env)
        found = {l.split()[0] for l in pr.stdout.splitlines() if l.endswith(" FOUND") and not l.endswith("NOT FOUND")}
        assert found == want, (with_e, pr.stdout)


def test_eth_kernels_keep_scratch_out_of_their_loops_and_the_which_loop_is_small():
    """static, from the assembly the build keeps (tools/isa_mix.py, ETH_KERNELS): each of the three ETH kernels has 128 or 168 VGPRs and no
    scratch instruction in a per-key loop (k_add_eth: every loop inside the launch loop - prefix products, table, `which`, and with -endo
    the image loop inside it; k_mul_check_eth: window, sum and walk-back loops).  The `which` loop of k_add_eth<false> - one key: curve
    arithmetic, normalisation, Keccak, probe 0 - is at most 5600 VALU instructions: ~770 for everything but the hash (the `which` loop of
    -a c less its hash160, profiles/r07_static_mix.json), ~35 for y, and a Keccak of at most 4800 (24 rounds x 200)."""
    import isa_mix
    ASM = kept_assembly()
    now = isa_mix.analyse_eth(ASM)
    assert set(now) == set(isa_mix.ETH_KERNELS) == {"-a e", "-a e -endo", "mul -a e"}
    for label, a in now.items():
        print(label, a["registers"], a["scratch_in_loops"], a["fingerprint"])
        assert a["registers"]["vgpr_count"] in (128, 168), (label, a["registers"])
        inner = {k: v for k, v in a["scratch_in_loops"].items() if k != "launch"}
        assert all(v == 0 for v in inner.values()), (label, a["scratch_in_loops"])
    # every loop below the launch loop of the two add kernels, whatever its depth (the image loop of -endo holds the Keccak)
    for label in ("-a e", "-a e -endo"):
        a = isa_mix.analyse(ASM, isa_mix.ETH_KERNELS[label])
        deep = [l for l in a["loops"] if l["depth"] >= 2]
        assert deep and all(l["scratch"] == 0 for l in deep), (label, [(l["header"], l["scratch"]) for l in deep])
        hashing = max(deep, key=lambda l: l["valu"])
        assert hashing["valu"] > 3000, (label, hashing)  # the loop that holds the Keccak was seen
    which = now["-a e"]["fingerprint"]["which_loop_valu"]
    print("which_loop_valu of k_add_eth<false>:", which)
    assert which <= 5600, which
