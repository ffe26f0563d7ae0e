#!/usr/bin/env python
"""Static instruction histogram of one kernel from hipcc's -S output, built with the Makefile's per-unit flags (as
tools/kernel_resources.py builds them).
usage: tools/kernel_insts.py UNIT KERNEL [--json] [--loops] [extra hipcc flags]
  UNIT    a kernel translation unit as the Makefile names it: gjk32, epa32, epa64, bvh, ...
  KERNEL  the kernel's name without template arguments (k_epa_loop); with several instantiations in the unit, the one whose
          demangled name contains every further word given as --match WORD

Instructions are classified by prefix only: v_ (VALU), s_ (SALU; branches, waits / s_nop and scalar memory reads apart), ds_ (LDS),
global_ / flat_ / buffer_ / scratch_ (vector memory); v_readlane / v_writelane -- the lane spills of SGPRs -- are a class of their
own (lane) and not VALU.  On top of the classes it counts the register copies (v_mov_b32 without a DPP or SDWA modifier) and the
64-bit mask instructions (s_*_b64).

Counted twice: for the whole kernel, and for its *trip loop*: among the loops of the kernel (a backward branch and everything
between it and its target, in layout order) the one with the most instructions that touches no memory but LDS.  A persistent kernel
that alternates between a phase on registers and LDS and a phase that reads its next work from memory has exactly one such loop
worth the name, whether the source spells it as a loop or the compiler's block placement makes it one; in a kernel without such a
phase it is the largest of the small scan loops.  --loops lists every loop."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("VALU", "lane", "SALU", "SMEM", "branch", "wait", "LDS", "VMEM", "other")
EXTRA = ("v_mov_b32", "v_cndmask", "lane_spill", "v_readlane", "v_writelane", "mask_b64", "s_cbranch_execz", "s_nop")


def unit_flags(unit):
    mk = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "hpp-fcl_amd", "csrc"), "-pn"], capture_output=True, text=True).stdout
    m = re.search(r"^FLAGS_k_%s = (.*)$" % unit, mk, re.M)
    return (m.group(1).split() if m else []) + (["-DHFCL_UNIT_PRECISION=" + unit[-2:]] if unit[-2:] in ("32", "64") else [])


def assembly(unit, flags):
    src = os.path.join(ROOT, "hpp-fcl_amd", "csrc", "hfcl_k_%s.hip" % unit.rstrip("0123456789"))
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-value", "-Wno-pass-failed",
               "--cuda-device-only", "-S", "-o", out, src] + unit_flags(unit) + flags
        subprocess.run(cmd, check=True, capture_output=True, text=True)
        with open(out) as f:
            return f.read().splitlines()


def classify(op):
    if op.startswith("s_cbranch") or op.startswith("s_branch") or op in ("s_setpc_b64", "s_swappc_b64"):
        return "branch"
    if op.startswith("s_waitcnt") or op == "s_nop":
        return "wait"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "SMEM"
    if op.startswith(("v_readlane", "v_writelane")):
        return "lane"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    return "other"


def histogram(ops):
    h = {c: 0 for c in CLASSES + EXTRA}
    for op in ops:
        h[classify(op)] += 1
        if op.startswith("v_mov_b32") and not op.endswith(("_dpp", "_sdwa")):  # (a DPP move is a cross-lane operation, not a copy)
            h["v_mov_b32"] += 1
        if op.startswith("v_cndmask"):
            h["v_cndmask"] += 1
        if op.startswith("v_readlane"):
            h["v_readlane"] += 1
        if op.startswith("v_writelane"):
            h["v_writelane"] += 1
        if classify(op) == "SALU" and re.search(r"_b64$", op):
            h["mask_b64"] += 1
        if op == "s_cbranch_execz":
            h["s_cbranch_execz"] += 1
        if op == "s_nop":
            h["s_nop"] += 1
    h["lane_spill"] = h["v_readlane"] + h["v_writelane"]
    h["total"] = len(ops)
    return h


def kernel_body(lines, kernel, words):
    """(mangled name, [(mnemonic, branch target or None) | label string]) of the one instantiation asked for"""
    found = []
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if not m:
            continue
        dem = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        if re.search(r"\b%s(<|\()" % re.escape(kernel), dem) and all(w in dem for w in words):
            found.append((i, m.group(1), dem))
    if len(found) != 1:
        sys.exit("kernel_insts: %d instantiations of %s match%s" % (len(found), kernel, "".join("\n  " + f[2] for f in found)))
    start, sym, dem = found[0]
    body = []
    for l in lines[start + 1:]:
        if re.match(r"^\.Lfunc_end\d+:", l):
            break
        m = re.match(r"^(\.L\w+):", l)
        if m:
            body.append(m.group(1))
            continue
        m = re.match(r"^\s+([a-z]\w*)\s*(.*?)\s*(?:;.*)?$", l)
        if m and not l.lstrip().startswith((".", ";")):
            t = re.search(r"(\.L\w+)", m.group(2)) if classify(m.group(1)) == "branch" else None
            body.append((m.group(1), t.group(1) if t else None))
    return dem, body


def loops_of(body):
    """[(first, last)] over the instruction indices of `body`'s instructions: one per loop header, the widest back edge"""
    at, ops, k = {}, [], 0
    for e in body:
        if isinstance(e, str):
            at[e] = k
        else:
            ops.append(e)
            k += 1
    spans = {}
    for i, (op, tgt) in enumerate(ops):
        if tgt is not None and tgt in at and at[tgt] <= i:
            spans[at[tgt]] = max(spans.get(at[tgt], i), i)
    return [o for o, _ in ops], sorted(spans.items())


def report(unit, kernel, words, flags):
    dem, body = kernel_body(assembly(unit, flags), kernel, words)
    ops, spans = loops_of(body)
    loops = []
    for a, b in spans:
        h = histogram(ops[a:b + 1])
        h["first"], h["last"] = a, b
        h["depth"] = sum(1 for c, d in spans if c <= a and b <= d and (c, d) != (a, b))
        loops.append(h)
    quiet = [l for l in loops if l["VMEM"] == 0 and l["SMEM"] == 0]
    trip = max(quiet, key=lambda l: l["total"]) if quiet else None
    return {"kernel": dem, "whole": histogram(ops), "trip_loop": trip, "loops": loops}


def main():
    args = sys.argv[1:]
    words, as_json, show_loops, rest = [], False, False, []
    while args:
        a = args.pop(0)
        if a == "--match":
            words.append(args.pop(0))
        elif a == "--json":
            as_json = True
        elif a == "--loops":
            show_loops = True
        else:
            rest.append(a)
    if len(rest) < 2:
        sys.exit(__doc__)
    r = report(rest[0], rest[1], words, rest[2:])
    if as_json:
        print(json.dumps(r))
        return
    print(r["kernel"])
    cols = ("total",) + CLASSES + EXTRA
    rows = [("whole kernel", r["whole"])] + ([("trip loop", r["trip_loop"])] if r["trip_loop"] else [])
    if show_loops:
        rows += [("loop @%d depth %d" % (l["first"], l["depth"]), l) for l in r["loops"]]
    print("%-22s" % "" + "".join(" %*s" % (max(6, len(c)), c) for c in cols))
    for name, h in rows:
        print("%-22s" % name + "".join(" %*d" % (max(6, len(c)), h[c]) for c in cols))


if __name__ == "__main__":
    main()
