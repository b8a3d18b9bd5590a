#!/usr/bin/env python3
"""Static instruction mix of the add kernel from the gfx950 assembly the build keeps next to the library
(ecloop_amd/libecloop_hip.gfx950.s, written by ecloop_amd/build.py with -save-temps: the assembly OF the shipped
code object, not a second compilation).

The compiler annotates every basic block with the loop it belongs to, so the blocks can be attributed to the loop
nest of k_add (add_kernel.h): launch loop > {prefix-product loop, table loop > `which` loop > probe loop}.
VALU instructions are split into the issue classes the microbenchmark (ecloop_amd/csrc/tools/ubench.hip ->
profiles/ubench_r02.txt) prices differently:
  mad64 : v_mad_u64_u32
  fast  : add / sub / and / or / xor / mov / not and v_bitop3_b32 - the opcodes that reach ~2.3-2.5 SIMD-cycles per
          wave64 instruction in long runs (and ~4.2 when single between other instructions)
  other : every other VALU instruction (rotates, shifts, v_add3, v_perm, multiplies, carries, selects, ...): >= 4.1
What the numbers are used for:
  * `fingerprint`: bench.py puts it into its JSON line and compares it with the one stored in
    profiles/r02_roofline.json (the PMC counters in that file belong to a particular build); the CPU test
    tests/test_profiles_fresh.py fails when a freshly built library drifts more than 1 % from it;
  * `per_key_static`: one trip of the `which` loop (one key; this includes its rarely executed candidate-ring
    blocks, so it is an UPPER estimate) + half a trip of the table loop around it and of the prefix-product loop
    (each serves two keys).  The PMC count SQ_INSTS_VALU is the truth for the total; the class SHARES come from here.

usage: tools/isa_mix.py [file.s] [mangled kernel name] [--json]     |     tools/isa_mix.py --all   (every instantiation: profiles/rNN_static_mix.json)
       tools/isa_mix.py --eth   (the three Ethereum kernels)
       tools/isa_mix.py --tr    (the Taproot kernels: registers, loops, the static VALU counts of the tagged hash and the window loop)
       tools/isa_mix.py --pub   (the public-key kernels: registers, loops, the static per-key VALU count beside -a c's from the same assembly)
       tools/isa_mix.py --bsgs  (the kernels `bsgs` adds: the insert walk beside -a x's from the same assembly, the origin set-up kernel)
       tools/isa_mix.py --kangaroo  (the herd walk of `kangaroo`: registers, the two per-kangaroo loops, a jump's static count and the inversion's share by M)
       tools/isa_mix.py --splitkey  (the two verification kernels of the split-key search: registers, spills, static VALU count, scratch in the window loop)
       tools/isa_mix.py --seed  (the two kernels of `seed`: registers, the PBKDF2 iteration loop's static mix, code size, scratch and issue-cycle floor)
       tools/isa_mix.py --compare other.s [file.s]  (every kernel of both assemblies: instruction mix, registers, spills, LDS, scratch, kernarg size; which differ, which are new)"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "ecloop_amd", "libecloop_hip.gfx950.s")
K_ADD33 = "_Z5k_addILb1ELb0ELb0EEv8add_args"
FAST = {"v_add_u32", "v_sub_u32", "v_subrev_u32", "v_and_b32", "v_or_b32", "v_xor_b32", "v_mov_b32", "v_not_b32", "v_bitop3_b32"}
KEYS = ("valu", "mad64", "fast", "other", "salu", "smem", "vmem", "lds", "scratch", "call", "scratch_at_calls")


def classify(op):
    base = re.sub(r"_(e32|e64|sdwa|dpp)$", "", op)
    if base == "v_mad_u64_u32":
        return "mad64"
    return "fast" if base in FAST else "other"


def zero():
    return {k: 0 for k in KEYS}


def add_to(c, op):
    if op.startswith("v_"):
        c["valu"] += 1
        c[classify(op)] += 1
    elif op.startswith("scratch_"):
        c["scratch"] += 1
    elif op.startswith(("global_", "buffer_", "flat_")):
        c["vmem"] += 1
    elif op.startswith("ds_"):
        c["lds"] += 1
    elif op.startswith(("s_load", "s_buffer_load")):
        c["smem"] += 1
    elif op.startswith("s_"):
        c["salu"] += 1
        if op.startswith("s_swappc"):
            c["call"] += 1


def blocks(path, kernel):
    """-> list of {label, header, depth, counts}: the basic blocks of `kernel` with the innermost loop they are in"""
    s = open(path).read()
    a = s.index("\n" + kernel + ":")
    b = s.index(".Lfunc_end", a)
    out = []
    cur = {"label": "entry", "header": None, "depth": 0, "c": zero()}
    lines = s[a:b].split("\n")[2:]
    i = 0
    while i < len(lines):
        line = lines[i]
        m = re.match(r"(\.LBB\d+_\d+):|; %bb\.(\d+):", line)
        if m:
            out.append(cur)
            label = m.group(1) or ("bb." + m.group(2))
            cur = {"label": label, "header": None, "depth": 0, "c": zero()}
            # the loop comments of this block: on this line and the comment-only lines that follow
            j, text = i, line
            while j + 1 < len(lines) and re.match(r"\s+;", lines[j + 1]):
                j += 1
                text += "\n" + lines[j]
            mm = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", text)
            if mm:
                cur["header"], cur["depth"] = label.lstrip(".L"), int(mm.group(1))
            else:
                mm = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", text)
                if mm:
                    cur["header"], cur["depth"] = mm.group(1), int(mm.group(2))
            i = j + 1
            continue
        mm = re.match(r"\s+([a-z][a-z0-9_]+)", line)
        if mm:
            add_to(cur["c"], mm.group(1))
        i += 1
    out.append(cur)
    for blk in out:  # a block that calls an out-of-line function passes its arguments through scratch: not spill traffic of the loop it sits in
        if blk["c"]["call"]:
            blk["c"]["scratch_at_calls"], blk["c"]["scratch"] = blk["c"]["scratch"], 0
    return out, s[b : b + 4000]


def loop_tree(path, kernel):
    """parent header of every loop header (from the `Parent Loop` comments)"""
    s = open(path).read()
    a = s.index("\n" + kernel + ":")
    b = s.index(".Lfunc_end", a)
    parent, depth = {}, {}
    for m in re.finditer(r"^\.L(BB\d+_\d+):((?:[^\n]*\n\s+;)*[^\n]*)", s[a:b], re.M):
        text = m.group(0)
        d = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", text)
        if not d:
            continue
        h = m.group(1)
        depth[h] = int(d.group(1))
        ps = re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", text)
        parent[h] = max(ps, key=lambda p: int(p[1]))[0] if ps else None
    return parent, depth


def analyse(path=ASM, kernel=K_ADD33):
    bl, tail = blocks(path, kernel)
    parent, depth = loop_tree(path, kernel)
    total = zero()
    excl = {h: zero() for h in parent}
    for b in bl:
        for k in KEYS:
            total[k] += b["c"][k]
            if b["header"] in excl:
                excl[b["header"]][k] += b["c"][k]
    res = {"kernel": kernel, "total": total,
           "loops": [{"header": h, "depth": depth[h], "parent": parent[h], **excl[h]} for h in sorted(parent, key=lambda h: (depth[h], h))]}
    m = re.search(r"\.private_seg_size, (\d+)", tail)
    res["scratch_bytes_own"] = int(m.group(1)) if m else None
    m = re.search(r"\.num_vgpr, (?:max\()?(\d+)", tail)
    res["vgpr"] = int(m.group(1)) if m else None
    # the loop nest of k_add: launch loop (depth 1, with children) > table loop (depth 2, with children) > `which` loop
    kids = {h: [c for c in parent if parent[c] == h] for h in parent}
    launch = [h for h in parent if depth[h] == 1 and kids[h]]
    if launch:
        L = max(launch, key=lambda h: sum(excl[c]["valu"] for c in kids[h]))
        table = [c for c in kids[L] if kids[c]]
        prefix = [c for c in kids[L] if not kids[c]]
        if table:
            T = table[0]
            W = max(kids[T], key=lambda h: excl[h]["valu"])
            est = {k: float(excl[W][k]) + excl[T][k] / 2.0 for k in ("valu", "mad64", "fast", "other")}
            if prefix:
                P = max(prefix, key=lambda h: excl[h]["valu"])
                for k in est:
                    est[k] += excl[P][k] / 2.0
                res["prefix_loop"] = excl[P]
            res["which_loop"], res["table_loop"], res["launch_loop"] = excl[W], excl[T], excl[L]
            res["per_key_static"] = est
            res["fingerprint"] = {"kernel_valu": total["valu"], "which_loop_valu": excl[W]["valu"], "which_loop_mad64": excl[W]["mad64"],
                                  "which_loop_fast": excl[W]["fast"], "table_loop_valu": excl[T]["valu"],
                                  "prefix_loop_valu": res.get("prefix_loop", zero())["valu"], "scratch_instr": total["scratch"] + total["scratch_at_calls"]}
            try:
                sp = spills(path).get(kernel)
                if sp:
                    res["fingerprint"]["vgpr_spill_count"] = sp["vgpr_spill_count"]
                    res["fingerprint"]["scratch_bytes"] = sp["scratch_bytes"]
            except Exception:
                pass
    return res


K_MUL_CU = "_Z11k_mul_checkILb1ELb1EEvPKjjj4wtab8add_argsPjjj"


def analyse_mul(path=ASM, kernel=K_MUL_CU, nwin=10):
    """k_mul_check (mul_kernels.h): loop nest = {sum loop (one trip per scalar) > window loop (nwin - 2 trips per scalar: windows 0 and 1
    are added before it), walk-back loop (one trip per scalar: two field multiplications pairs + the hash160s + stage-1 probes; its
    children are the rarely taken ring-drain loops), three ring-flush loops after it}.  Per-scalar static estimate of the class mix =
    sum loop + (nwin - 2) x window loop + walk-back loop, each exclusive of its children (the inversion - one per thread, shared by the
    thread's scalars - and the out-of-line complete sum are left out: the PMC count is the truth for the total, the SHARES come from here)."""
    bl, _ = blocks(path, kernel)
    parent, depth = loop_tree(path, kernel)
    excl = {h: zero() for h in parent}
    total = zero()
    for b in bl:
        for k in KEYS:
            total[k] += b["c"][k]
            if b["header"] in excl:
                excl[b["header"]][k] += b["c"][k]
    kids = {h: [c for c in parent if parent[c] == h] for h in parent}
    top = [h for h in parent if depth[h] == 1]
    # the window loop: the depth-2 loop with the most multiply-adds; the sum loop is its parent; the walk-back loop: the hash-heavy one
    win = max((h for h in parent if depth[h] == 2), key=lambda h: excl[h]["mad64"])
    summ = parent[win]
    back = max((h for h in top if h != summ), key=lambda h: excl[h]["other"])
    est = {k: float(excl[summ][k]) + (nwin - 2) * excl[win][k] + excl[back][k] for k in ("valu", "mad64", "fast", "other")}
    return {"kernel": kernel, "total": total, "sum_loop": excl[summ], "window_loop": excl[win], "walk_back_loop": excl[back], "windows": nwin,
            "per_scalar_static": est,
            "fingerprint": {"kernel_valu": total["valu"], "window_loop_valu": excl[win]["valu"], "window_loop_mad64": excl[win]["mad64"],
                            "walk_back_loop_valu": excl[back]["valu"], "scratch_instr": total["scratch"] + total["scratch_at_calls"],
                            "window_loop_scratch": excl[win]["scratch"]}}


def spills(path=ASM, prefix="_Z5k_add"):
    """vgpr_spill_count / private_segment_fixed_size / vgpr_count of every instantiation of the add kernel, from the code
    object's metadata (DESIGN.md states these numbers; tests/test_profiles_fresh.py compares)"""
    s = open(path).read()
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\n(?=  - \.agpr_count:|amdhsa\.target|\.\.\.)", s, re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or not name.group(1).startswith(prefix):
            continue
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
        out[name.group(1)] = {"vgpr_count": g("vgpr_count"), "vgpr_spill_count": g("vgpr_spill_count"),
                              "scratch_bytes": g("private_segment_fixed_size")}
    return out


ADD_KERNELS = {"-a c": "_Z5k_addILb1ELb0ELb0EEv8add_args", "-a u": "_Z5k_addILb0ELb1ELb0EEv8add_args", "-a cu": "_Z5k_addILb1ELb1ELb0EEv8add_args",
               "-a c -endo": "_Z5k_addILb1ELb0ELb1EEv8add_args", "-a u -endo": "_Z5k_addILb0ELb1ELb1EEv8add_args", "-a cu -endo": "_Z5k_addILb1ELb1ELb1EEv8add_args"}
MUL_KERNELS = {"mul -a c": "_Z11k_mul_checkILb1ELb0EEvPKjjj4wtab8add_argsPjjj", "mul -a u": "_Z11k_mul_checkILb0ELb1EEvPKjjj4wtab8add_argsPjjj",
               "mul -a cu": K_MUL_CU}


# the Ethereum kernels (-a e, searched alone): a dictionary of their own - ADD_KERNELS / MUL_KERNELS are the sets the tracked profiles cover
ETH_KERNELS = {"-a e": "_Z9k_add_ethILb0EEv8add_args", "-a e -endo": "_Z9k_add_ethILb1EEv8add_args",
               "mul -a e": "_Z15k_mul_check_ethPKjjj4wtab8add_argsPjjj"}


def analyse_eth(path=ASM):
    """the three ETH kernels in analyse_all's form (tests/test_eth_host.py: no scratch in the per-key loops, the `which` loop's size)"""
    sp = {**spills(path, "_Z9k_add_eth"), **spills(path, "_Z15k_mul_check_eth")}
    out = {}
    for label, k in ETH_KERNELS.items():
        if "k_mul_check" in k:
            m = analyse_mul(path, k)
            out[label] = {"kernel": k, "fingerprint": m["fingerprint"], "registers": sp.get(k),
                          "scratch_in_loops": {"window": m["window_loop"]["scratch"], "sum": m["sum_loop"]["scratch"], "walk_back": m["walk_back_loop"]["scratch"]},
                          "per_scalar_static": {x: round(v, 1) for x, v in m["per_scalar_static"].items()}}
        else:
            a = analyse(path, k)
            out[label] = {"kernel": k, "fingerprint": a["fingerprint"], "registers": sp.get(k),
                          "scratch_in_loops": {"which": a["which_loop"]["scratch"], "table": a["table_loop"]["scratch"], "prefix": a["prefix_loop"]["scratch"],
                                               "launch": a["launch_loop"]["scratch"]},
                          "per_key_static": {x: round(v, 1) for x, v in a["per_key_static"].items()}}
    return out


# the prefix kernels (-p): the walk and the hashes of k_add / k_add_eth with the prefix filter (csrc/prefix.h) and one ring
PREFIX_KERNELS = {"-p -a c": "_Z9k_add_pfxILb1ELb0ELb0EEv8add_args", "-p -a u": "_Z9k_add_pfxILb0ELb1ELb0EEv8add_args", "-p -a cu": "_Z9k_add_pfxILb1ELb1ELb0EEv8add_args",
                  "-p -a c -endo": "_Z9k_add_pfxILb1ELb0ELb1EEv8add_args", "-p -a u -endo": "_Z9k_add_pfxILb0ELb1ELb1EEv8add_args",
                  "-p -a cu -endo": "_Z9k_add_pfxILb1ELb1ELb1EEv8add_args", "-p -a e": "_Z13k_add_pfx_ethILb0EEv8add_args", "-p -a e -endo": "_Z13k_add_pfx_ethILb1EEv8add_args"}


def analyse_prefix(path=ASM):
    """the eight prefix kernels in analyse_all's form"""
    sp = {**spills(path, "_Z9k_add_pfx"), **spills(path, "_Z13k_add_pfx_eth")}
    out = {}
    for label, k in PREFIX_KERNELS.items():
        a = analyse(path, k)
        out[label] = {"kernel": k, "fingerprint": a["fingerprint"], "registers": sp.get(k),
                      "scratch_in_loops": {"which": a["which_loop"]["scratch"], "table": a["table_loop"]["scratch"], "prefix": a["prefix_loop"]["scratch"],
                                           "launch": a["launch_loop"]["scratch"]},
                      "per_key_static": {x: round(v, 1) for x, v in a["per_key_static"].items()}}
    return out


# the mask kernels (-p 0xdead*beef -a e): the walk and Keccak of k_add_pfx_eth with the mask filter (csrc/mask.h); beside each the prefix kernel
# it mirrors, from the same assembly
MASK_KERNELS = {"-p mask -a e": "_Z13k_add_msk_ethILb0EEv8add_args", "-p mask -a e -endo": "_Z13k_add_msk_ethILb1EEv8add_args"}
MASK_MIRRORS = {"-p mask -a e": "_Z13k_add_pfx_ethILb0EEv8add_args", "-p mask -a e -endo": "_Z13k_add_pfx_ethILb1EEv8add_args"}


def analyse_mask(path=ASM):
    """the two mask kernels and the prefix kernels they mirror: metadata (registers, spills, scratch, LDS), fingerprint, loops"""
    meta = kernel_meta(path)
    out = {}
    for label, k in MASK_KERNELS.items():
        r = {}
        for tag, name in (("kernel", k), ("mirror", MASK_MIRRORS[label])):
            a = analyse(path, name)
            r[tag] = {"name": name, "registers": meta.get(name), "fingerprint": a["fingerprint"], "total": a["total"],
                      "scratch_in_loops": {"which": a["which_loop"]["scratch"], "table": a["table_loop"]["scratch"], "prefix": a["prefix_loop"]["scratch"],
                                           "launch": a["launch_loop"]["scratch"]},
                      "loops": [{x: l[x] for x in ("header", "depth", "parent", "valu", "salu", "smem", "vmem", "lds", "scratch")} for l in a["loops"]],
                      "per_key_static": {x: round(v, 1) for x, v in a["per_key_static"].items()}}
        out[label] = r
    return out


# the Taproot kernels (-a t, searched alone): stage A (the emit kernels from the walk and from `mul`'s window sums) and stage B (k_tr_check;
# <true>: ecl_hip_diag_tr's instantiation, which writes whole output keys instead of probing)
TR_KERNELS = {"-a t emit": "_Z8k_add_tr8add_args", "mul -a t emit": "_Z15k_mul_points_trPKjjj4wtab8add_argsPjjj",
              "tr check": "_Z10k_tr_checkILb0EEvPKjjm4wtab8add_argsjPjjjS4_Ph", "tr check (diag)": "_Z10k_tr_checkILb1EEvPKjjm4wtab8add_argsjPjjjS4_Ph"}


def analyse_tr(path=ASM):
    """every Taproot kernel: registers / spills, its loops (depth, VALU, scratch), `scratch_below_top`: scratch instructions in the loops below
    its launch loop (k_add_tr) / round loops (the others) - tests/test_tr_host.py wants 0 - and `scratch_in_round_loops` for the `mul`-shaped
    kernels; the static VALU count of the loop that holds the tagged hash (the emit kernels: the `which` loop / the walk-back loop) and of
    the window loop (one mixed addition)"""
    out = {}
    for label, k in TR_KERNELS.items():
        a = analyse(path, k)
        sp = spills(path, k).get(k)
        loops = a["loops"]
        deep = [l for l in loops if l["depth"] >= 2]
        top = [l for l in loops if l["depth"] == 1]
        r = {"kernel": k, "registers": sp, "total": a["total"],
             "loops": [{x: l[x] for x in ("header", "depth", "parent", "valu", "mad64", "scratch", "scratch_at_calls")} for l in loops],
             "scratch_below_top": sum(l["scratch"] for l in deep)}
        if label == "-a t emit":
            r["tagged_hash_loop_valu"] = a["which_loop"]["valu"]
        else:
            r["scratch_in_round_loops"] = sum(l["scratch"] for l in top)
            win = max(deep, key=lambda l: l["mad64"])
            r["window_loop_valu"], r["window_loop_mad64"] = win["valu"], win["mad64"]
            back = max((l for l in top if l["header"] != win["parent"]), key=lambda l: l["valu"])
            r["walk_back_loop_valu"] = back["valu"]
        out[label] = r
    return out


# the public-key kernels (-a x, searched alone): the walk with x-only emission and `mul`'s body with x alone; a dictionary of their own
PUB_KERNELS = {"-a x": "_Z9k_add_pubILb0EEv8add_args", "-a x -endo": "_Z9k_add_pubILb1EEv8add_args",
               "mul -a x": "_Z15k_mul_check_pubPKjjj4wtab8add_argsPjjj"}
HASH160_VALU = 2248  # the two compression functions of one hash160, VALU lane-ops per key


def analyse_pub(path=ASM):
    """every public-key kernel: registers / spills, its loops (depth, VALU, scratch), `scratch_below_top`: scratch instructions in the loops
    below its launch loop (k_add_pub) / round loops (k_mul_check_pub) - tests/test_pub_host.py wants 0; for the walk kernels the static
    per-key VALU count (`which` loop + half the table loop's own body + half the prefix loop), and beside it `-a c`'s from the same assembly
    and that figure less the hash160: the hash must be gone"""
    out = {}
    ref = analyse(path, K_ADD33)["per_key_static"]["valu"]
    for label, k in PUB_KERNELS.items():
        a = analyse(path, k)
        sp = spills(path, k).get(k)
        loops = a["loops"]
        deep = [l for l in loops if l["depth"] >= 2]
        r = {"kernel": k, "registers": sp, "total": a["total"],
             "loops": [{x: l[x] for x in ("header", "depth", "parent", "valu", "mad64", "scratch", "scratch_at_calls")} for l in loops],
             "scratch_below_top": sum(l["scratch"] for l in deep)}
        if "k_add_pub" in k:
            r["which_loop_valu"], r["table_loop_valu"], r["prefix_loop_valu"] = a["which_loop"]["valu"], a["table_loop"]["valu"], a["prefix_loop"]["valu"]
            r["per_key_valu"] = a["per_key_static"]["valu"]
            r["addr33_per_key_valu"], r["addr33_less_hash160"] = ref, ref - HASH160_VALU
            if "ILb1E" in k:  # -endo: the loop over the three x values (one probe each), the child of the `which` loop that has children itself
                which = max((l for l in loops if l["depth"] == 3), key=lambda l: l["valu"])["header"]
                kids = [l for l in loops if l["parent"] == which and any(c["parent"] == l["header"] for c in loops)]
                r["image_loop_valu"] = max((l["valu"] for l in kids), default=None)
        else:
            m = analyse_mul(path, k)
            r["scratch_in_round_loops"] = sum(l["scratch"] for l in loops if l["depth"] == 1)
            r["window_loop_valu"], r["window_loop_mad64"], r["walk_back_loop_valu"] = m["window_loop"]["valu"], m["window_loop"]["mad64"], m["walk_back_loop"]["valu"]
        out[label] = r
    return out


# the kernels `bsgs` adds: the insert walk of the baby table (the giant walk runs k_add_pub<false> itself) and the one-thread origin shift
BSGS_KERNELS = {"bsgs insert": "_Z13k_add_pub_ins8add_args", "bsgs origin": "_Z12k_origin_addPj10origin_argS_"}


def analyse_bsgs(path=ASM):
    """the insert walk in analyse_pub's form - registers / spills, loops, `scratch_below_top`, the static per-key VALU count (the 20 atomic
    ORs of a key are VMEM, counted in `which_loop_vmem`) beside -a x's from the same assembly - and the registers of the origin kernel"""
    k = BSGS_KERNELS["bsgs insert"]
    a = analyse(path, k)
    loops = a["loops"]
    r = {"kernel": k, "registers": spills(path, k).get(k), "total": a["total"],
         "loops": [{x: l[x] for x in ("header", "depth", "parent", "valu", "mad64", "vmem", "scratch", "scratch_at_calls")} for l in loops],
         "scratch_below_top": sum(l["scratch"] for l in loops if l["depth"] >= 2),
         "which_loop_valu": a["which_loop"]["valu"], "which_loop_vmem": a["which_loop"]["vmem"], "table_loop_valu": a["table_loop"]["valu"],
         "prefix_loop_valu": a["prefix_loop"]["valu"], "per_key_valu": a["per_key_static"]["valu"],
         "pub_per_key_valu": analyse(path, PUB_KERNELS["-a x"])["per_key_static"]["valu"]}
    o = BSGS_KERNELS["bsgs origin"]
    return {"bsgs insert": r, "bsgs origin": {"kernel": o, "registers": spills(path, o).get(o)}}


# the kernels `kangaroo` adds: the herd walk and the set-up of its starts
HERD_KERNELS = {"herd walk": "_Z11k_herd_walk9herd_args", "herd init": "_Z11k_herd_initPKjPKhS0_6herd_qPjjjjS4_"}
INV_VALU_DYNAMIC = 16400  # fe_inv's executed VALU instructions (the figure ecloop_hip.hip's inv_keys_worth uses)


def analyse_herd(path=ASM):
    """the herd walk: registers / spills, its loop nest (step loop > pass 1, pass 2), the scratch instructions inside the two per-kangaroo
    loops, the static VALU count of a jump (both passes' bodies, rare paths included) and, for M = 16, 32, 64 kangaroos per lane, the
    inversion's share of a jump"""
    k = HERD_KERNELS["herd walk"]
    bl, _ = blocks(path, k)
    parent, depth = loop_tree(path, k)
    excl = {h: zero() for h in parent}
    for b in bl:
        if b["header"] in excl:
            for key in KEYS:
                excl[b["header"]][key] += b["c"][key]
    inner = sorted((h for h in parent if depth[h] == 2), key=lambda h: excl[h]["valu"])
    r = {"kernel": k, "registers": spills(path, k).get(k),
         "loops": [{"header": h, "depth": depth[h], "parent": parent[h], **{x: excl[h][x] for x in ("valu", "mad64", "vmem", "lds", "scratch")}}
                   for h in sorted(parent, key=lambda h: (depth[h], h))]}
    if len(inner) >= 2:
        p1, p2 = excl[inner[0]], excl[inner[-1]]
        jump = p1["valu"] + p2["valu"]
        r.update({"pass1_valu": p1["valu"], "pass2_valu": p2["valu"], "jump_valu": jump, "scratch_in_passes": p1["scratch"] + p2["scratch"],
                  "lds_in_passes": p1["lds"] + p2["lds"], "vmem_in_passes": p1["vmem"] + p2["vmem"],
                  "per_jump_with_inversion": {m: round(jump + INV_VALU_DYNAMIC / m) for m in (16, 32, 64)},
                  "inversion_share": {m: round(INV_VALU_DYNAMIC / m / (jump + INV_VALU_DYNAMIC / m), 3) for m in (16, 32, 64)}})
    o = HERD_KERNELS["herd init"]
    return {"herd walk": r, "herd init": {"kernel": o, "registers": spills(path, o).get(o)}}


# the kernels the split-key search adds (-p with -k): the re-derivation of a hit, O + k G by the window-table sum and one more complete addition
SPLITKEY_KERNELS = {"verify origin": "_Z15k_verify_originPKjjS0_PjS1_Ph", "verify origin eth": "_Z19k_verify_origin_ethPKjjS0_PjPh"}
SPLITKEY_MIRRORS = {"verify origin": "_Z8k_verifyPKjjS0_PjS1_Ph", "verify origin eth": "_Z12k_verify_ethPKjjS0_PjPh"}


# the kernels `seed` adds (ECL_KDF_BIP39): the master stage (PBKDF2-HMAC-SHA512 + the master node) and the path stage (CKDpriv)
SEED_KERNELS = {"master": "_Z14k_bip39_masterPKjjPKmj10bip39_saltPj", "path": "_Z12k_bip32_pathPKjj10bip32_pathS0_Pj"}
SEED_ROUND_PASSES = 4      # a compression's rounds 16..79: four passes over the body of 16
SEED_ITERATIONS = 2047     # of the loop (PBKDF2's 2048 minus U_1)
SEED_CLOCKS = {"fast": 2.4, "other": 4.1}  # DESIGN section 4's measured issue clocks per wave instruction
SEED_SIMDS, SEED_HZ = 1024, 2.4e9


def analyse_seed(path=ASM):
    """k_bip39_master's iteration loop - the depth-1 loop that holds two round loops, one per compression of an HMAC - and what an iteration
    executes: its own body once and each round loop four times.  Its instructions are at most 8 bytes each (gfx950 has no literal in VOP3), which
    bounds the loop's code size.  The issue-cycle floor as DESIGN (f14) computed camp2's: the loop's VALU mix at 2.4 / 4.1 clocks, 64
    phrases a wave, 1024 SIMDs at 2.4 GHz.  Beside it the registers of both kernels."""
    meta = kernel_meta(path)
    k = SEED_KERNELS["master"]
    bl, _ = blocks(path, k)
    parent, depth = loop_tree(path, k)
    excl = {h: zero() for h in parent}
    ninstr = {h: 0 for h in parent}
    for b in bl:
        if b["header"] in excl:
            for key in KEYS:
                excl[b["header"]][key] += b["c"][key]
            ninstr[b["header"]] += sum(b["c"][x] for x in ("valu", "salu", "smem", "vmem", "lds", "scratch"))
    kids = {h: [c for c in parent if parent[c] == h] for h in parent}
    cands = [h for h in parent if depth[h] == 1 and len(kids[h]) == 2 and not excl[h]["vmem"]]
    r = {"master": {"kernel": k, "registers": meta.get(k), "loops": len(parent)}, "path": {"kernel": SEED_KERNELS["path"], "registers": meta.get(SEED_KERNELS["path"])}}
    if len(cands) == 1:
        L = cands[0]
        dyn = {x: excl[L][x] + SEED_ROUND_PASSES * sum(excl[c][x] for c in kids[L]) for x in ("valu", "fast", "other", "mad64", "salu", "smem")}
        clocks = dyn["fast"] * SEED_CLOCKS["fast"] + (dyn["other"] + dyn["mad64"]) * SEED_CLOCKS["other"]
        per_phrase = clocks * SEED_ITERATIONS / 64.0
        r["master"]["iteration_loop"] = {
            "header": L, "own": {x: excl[L][x] for x in ("valu", "fast", "other", "scratch", "vmem", "lds")},
            "round_loops": [{x: excl[c][x] for x in ("valu", "fast", "other", "scratch", "vmem", "lds", "smem")} for c in sorted(kids[L])],
            "scratch": excl[L]["scratch"] + excl[L]["scratch_at_calls"] + sum(excl[c]["scratch"] + excl[c]["scratch_at_calls"] for c in kids[L]),
            "calls": excl[L]["call"] + sum(excl[c]["call"] for c in kids[L]),
            "instructions": ninstr[L] + sum(ninstr[c] for c in kids[L]), "code_bytes_max": 8 * (ninstr[L] + sum(ninstr[c] for c in kids[L])),
            "per_iteration": dyn, "valu_per_compression": dyn["valu"] / 2.0, "clocks_per_iteration": round(clocks, 1),
            "floor_phrases_per_s": round(SEED_SIMDS * SEED_HZ / per_phrase)}
    return r


def kernel_meta(path=ASM):
    """name -> the code object's metadata of every kernel: register counts, spill counts, scratch, LDS and kernarg sizes"""
    s = open(path).read()
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\n(?=  - \.agpr_count:|amdhsa\.target|\.\.\.)", s, re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
        out[name.group(1)] = {k: g(k) for k in ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                                "group_segment_fixed_size", "kernarg_segment_size")}
    return out


def kernel_table(path=ASM):
    """name -> metadata + the static instruction mix of every kernel of the assembly"""
    out = {}
    for name, meta in kernel_meta(path).items():
        bl, _ = blocks(path, name)
        total = zero()
        for b in bl:
            for k in KEYS:
                total[k] += b["c"][k]
        out[name] = {**meta, **total}
    return out


def compare(other, path=ASM):
    """the kernels of `path` against those of `other` (the parent's build): identical, different (with both rows), new, gone"""
    a, b = kernel_table(other), kernel_table(path)
    return {"kernels_other": len(a), "kernels": len(b), "identical": sum(1 for k in a if k in b and a[k] == b[k]),
            "different": {k: {"other": a[k], "this": b[k]} for k in a if k in b and a[k] != b[k]},
            "new": sorted(k for k in b if k not in a), "gone": sorted(k for k in a if k not in b)}


def analyse_splitkey(path=ASM):
    """the two verification kernels beside the kernels whose bodies they are (k_verify, k_verify_eth) from the same assembly: registers /
    spills / scratch, the static instruction mix, their loops (the window loop is the one with the multiply-adds: the sum of table points)
    and the scratch instructions inside it - tests/test_splitkey_host.py wants 0"""
    meta = kernel_meta(path)
    out = {}
    for label, k in SPLITKEY_KERNELS.items():
        r = {}
        for tag, name in (("kernel", k), ("mirror", SPLITKEY_MIRRORS[label])):
            a = analyse(path, name)
            loops = [{x: l[x] for x in ("header", "depth", "parent", "valu", "mad64", "vmem", "scratch", "scratch_at_calls")} for l in a["loops"]]
            win = max(loops, key=lambda l: l["mad64"]) if loops else None
            r[tag] = {"name": name, "registers": meta.get(name), "total": a["total"], "loops": loops,
                      "window_loop": win, "window_loop_scratch": win["scratch"] if win else None}
        out[label] = r
    return out


def analyse_all(path=ASM):
    """every shipped instantiation of the two search kernels: fingerprint, registers / spills, and the scratch instructions inside the
    per-key loops (k_add: prefix-product, table and `which` loops; k_mul_check: window loop) - tests/test_profiles_fresh.py wants 0 there"""
    sp_add, sp_mul = spills(path), spills(path, "_Z11k_mul_check")
    out = {}
    for label, k in ADD_KERNELS.items():
        a = analyse(path, k)
        out[label] = {"kernel": k, "fingerprint": a["fingerprint"], "registers": sp_add.get(k),
                      "scratch_in_loops": {"which": a["which_loop"]["scratch"], "table": a["table_loop"]["scratch"], "prefix": a["prefix_loop"]["scratch"],
                                           "launch": a["launch_loop"]["scratch"]},
                      "per_key_static": {x: round(v, 1) for x, v in a["per_key_static"].items()}}
    for label, k in MUL_KERNELS.items():
        m = analyse_mul(path, k)
        out[label] = {"kernel": k, "fingerprint": m["fingerprint"], "registers": sp_mul.get(k),
                      "scratch_in_loops": {"window": m["window_loop"]["scratch"], "sum": m["sum_loop"]["scratch"], "walk_back": m["walk_back_loop"]["scratch"],
                                           "sum_at_the_call_of_the_complete_sum": m["sum_loop"]["scratch_at_calls"]},
                      "per_scalar_static": {x: round(v, 1) for x, v in m["per_scalar_static"].items()}}
    return out


def main():
    if "--eth" in sys.argv:
        rest = [a for a in sys.argv[1:] if not a.startswith("--")]
        print(json.dumps(analyse_eth(rest[0] if rest else ASM), indent=1))
        return
    if "--prefix" in sys.argv:
        rest = [a for a in sys.argv[1:] if not a.startswith("--")]
        print(json.dumps(analyse_prefix(rest[0] if rest else ASM), indent=1))
        return
    if "--mask" in sys.argv:
        rest = [a for a in sys.argv[1:] if not a.startswith("--")]
        print(json.dumps(analyse_mask(rest[0] if rest else ASM), indent=1))
        return
    if "--tr" in sys.argv:
        rest = [a for a in sys.argv[1:] if not a.startswith("--")]
        print(json.dumps(analyse_tr(rest[0] if rest else ASM), indent=1))
        return
    if "--pub" in sys.argv:
        rest = [a for a in sys.argv[1:] if not a.startswith("--")]
        print(json.dumps(analyse_pub(rest[0] if rest else ASM), indent=1))
        return
    if "--bsgs" in sys.argv:
        rest = [a for a in sys.argv[1:] if not a.startswith("--")]
        print(json.dumps(analyse_bsgs(rest[0] if rest else ASM), indent=1))
        return
    if "--kangaroo" in sys.argv:
        rest = [a for a in sys.argv[1:] if not a.startswith("--")]
        print(json.dumps(analyse_herd(rest[0] if rest else ASM), indent=1))
        return
    if "--splitkey" in sys.argv:
        rest = [a for a in sys.argv[1:] if not a.startswith("--")]
        print(json.dumps(analyse_splitkey(rest[0] if rest else ASM), indent=1))
        return
    if "--seed" in sys.argv:
        rest = [a for a in sys.argv[1:] if not a.startswith("--")]
        print(json.dumps(analyse_seed(rest[0] if rest else ASM), indent=1))
        return
    if "--compare" in sys.argv:
        rest = [a for a in sys.argv[1:] if not a.startswith("--")]
        print(json.dumps(compare(rest[0], rest[1] if len(rest) > 1 else ASM), indent=1))
        return
    if "--all" in sys.argv:
        rest = [a for a in sys.argv[1:] if not a.startswith("--")]
        print(json.dumps(analyse_all(rest[0] if rest else ASM), indent=1))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else ASM
    kernel = args[1] if len(args) > 1 else K_ADD33
    if "k_mul_check" in kernel:
        a = analyse_mul(path, kernel)
        print(json.dumps(a, indent=1) if "--json" in sys.argv else "%s\nper scalar (static, %d windows): %s\nfingerprint: %s" % (
            kernel, a["windows"], {k: round(v, 1) for k, v in a["per_scalar_static"].items()}, a["fingerprint"]))
        return
    a = analyse(path, kernel)
    if "--json" in sys.argv:
        print(json.dumps(a, indent=1))
        return
    t = a["total"]
    print("%s: %d VALU (%d mad64, %d fast, %d other), %d SALU, %d VMEM, %d SMEM, %d LDS, %d scratch instr; %s VGPRs, %s B scratch (own)" %
          (kernel, t["valu"], t["mad64"], t["fast"], t["other"], t["salu"], t["vmem"], t["smem"], t["lds"], t["scratch"],
           a["vgpr"], a["scratch_bytes_own"]))
    for l in a["loops"]:
        print("  %sloop %-10s (in %s): VALU %5d  mad64 %4d  fast %4d  other %5d  vmem %d lds %d scratch %d" %
              ("  " * (l["depth"] - 1), l["header"], l["parent"], l["valu"], l["mad64"], l["fast"], l["other"], l["vmem"], l["lds"], l["scratch"]))
    if "per_key_static" in a:
        print("per key (static, upper estimate): %s" % {k: round(v, 1) for k, v in a["per_key_static"].items()})
        print("fingerprint: %s" % a["fingerprint"])
    for k, v in sorted(spills(path).items()):
        print("  %s: %s" % (k, v))


if __name__ == "__main__":
    main()
