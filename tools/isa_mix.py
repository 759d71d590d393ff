#!/usr/bin/env python3
"""tools/isa_mix.py [--json OUT] [--label L] [-D MACRO[=V] ...] [NAME ...] -- static instruction accounting of k_brent.

Compiles named k_brent instantiations to gfx950 assembly with the Makefile's flags (hipcc -S --cuda-device-only; no GPU
needed, a few seconds each) and reports the instruction mix -- VALU, SALU, branches, s_load_*, s_waitcnt lgkmcnt, LDS,
vector memory -- of the whole kernel and of two regions:

  brent_loop   the cycle inside the item loop that holds wave_prod's row_bcast DPP steps: one objective evaluation and
               one Brent update.  Found from the control flow graph, so it needs no marker.
  hoist_slot   one slot row of the QUAD hoisting, between the assembler comments the source emits under -DPM_ISA_MARK
               ("; PM_MARK hoist_dn_slot_begin" / "_end", at hoist_quad_t's scheduling barriers): the per-slot list
               and its median, and per slot the path a full slot row executes (the cheapest path through the slot's
               blocks: it branches around the clamped DMA addresses and the phantom family) with its VALU and
               s_load counts and every s_waitcnt lgkmcnt on it: its count, the LDS / scalar loads it retires and
               the number of VALU instructions between the last of those and the wait ("valu_gap": 0 = the wave
               sits in the wait with nothing behind it; "ring_gap": the same from the last ring read it retires).

The markers must not change the code: every instantiation is compiled with and without -DPM_ISA_MARK and the two
whole-kernel and brent_loop mixes are compared ("markers_neutral").  The figures are static counts: the executed count
of a region is its static count only where the region is straight-line code (a hoisting slot); the Brent loop holds
both update branches, so its executed path is shorter than its static size.

The tool accounts for instruction classes only.  NAME: headline (64 x 16 QUAD --denovo), plain128 (128 x 16 plain PF, split trio / quad plan),
or a k_brent template argument list in quotes.  -D switches (PM_SERIAL_V0=1: the earlier serial path; PM_QD_PIPE=0: the
earlier QUAD hoisting) reach the compile.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polymutt_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# polymutt_amd/Makefile: COMMON + HIPFLAGS (warnings off)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w", "--offload-arch=gfx950", "-munsafe-fp-atomics"]
NAMES = {
    "headline": "64, 16, PM_NUM_POLY, false, false, true, false, false, true, 0, 8",
    "plain128": "128, 16, PM_NUM_POLY, false, false, false, true, false, false, 34, 8",
}
CLASSES = ("valu", "salu", "branch", "s_load", "waitcnt_lgkm", "lds", "vmem", "other")
_NOT_SALU = ("s_waitcnt", "s_nop", "s_endpgm", "s_barrier", "s_sleep", "s_setprio", "s_sethalt", "s_code_end", "s_inst_prefetch",
             "s_icache_inv", "s_trap")


def classify(op, line):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_load_") or op.startswith("s_buffer_load_"):
        return "s_load"
    if op.startswith("s_branch") or op.startswith("s_cbranch"):
        return "branch"
    if op == "s_waitcnt":
        return "waitcnt_lgkm" if "lgkmcnt" in line else "other"
    if op.startswith("ds_"):
        return "lds"
    if op.split("_")[0] in ("global", "buffer", "flat", "scratch"):
        return "vmem"
    if op.startswith("s_") and not op.startswith(_NOT_SALU):
        return "salu"
    return "other"


def compile_asm(targs, defines):
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "k.hip"), os.path.join(d, "k.s")
        with open(src, "w") as f:
            f.write('#define PM_BRENT_PART 0\n#include "engine_dev.h"\n'
                    f"template __global__ void k_brent<{targs}>(DevArgs, int);\n")
        cmd = [HIPCC, *FLAGS, *[f"-D{x}" for x in defines], "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-S",
               "--cuda-device-only", "-x", "hip", src, "-o", out]
        subprocess.run(cmd, check=True)
        return open(out).read()


def kernel_lines(text):
    """The lines of the (one) k_brent function, and its resource figures from the metadata comments."""
    lines = text.splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"_Z7k_brent\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    res = {}
    for key, pat in (("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
                     ("lds_static", r"; LDSByteSize: (\d+)")):
        m = re.search(pat, text)
        res[key] = int(m.group(1)) if m else None
    return lines[start + 1:end], res


def blocks(lines):
    """The function's basic blocks in layout order: label, whether the compiler marks it the header of a top-level
    (depth 1) loop, its instruction lines and its successors (branch targets and the fall-through)."""
    out, cur = [], None
    for l in lines:
        m = re.match(r"(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)\s*(;.*)?$", l)
        if m:
            cur = {"label": m.group(1) or "bb." + m.group(2), "note": [m.group(3) or ""], "ins": []}
            out.append(cur)
        elif cur is None:
            continue
        elif re.match(r"\s+;", l) and not cur["ins"] and "PM_MARK" not in l:
            cur["note"].append(l.strip())
        elif (l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;")) or "PM_MARK" in l:
            cur["ins"].append(l.strip())
    for i, b in enumerate(out):
        b["top_header"] = bool(re.search(r"Loop Header: Depth=1\b", " ".join(b["note"])))
        real = [x for x in b["ins"] if not x.startswith(";")]
        b["succ"] = [m.group(1) for x in real for m in [re.match(r"s_c?branch\w*\s+\.L(BB\d+_\d+)", x)] if m]
        if i + 1 < len(out) and not (real and real[-1].split()[0] in ("s_branch", "s_endpgm")):
            b["succ"].append(out[i + 1]["label"])
    return out


def mix(ins):
    c = dict.fromkeys(CLASSES, 0)
    for l in ins:
        if l.startswith(";"):
            continue
        c[classify(l.split()[0], l)] += 1
    return c


def brent_loop(bl):
    """The Brent loop: the cycle inside the item loop that holds wave_prod's row_bcast DPP steps.  Taken from the control
    flow graph -- the strongly connected component of a row_bcast block once the top-level loop headers are removed --
    because the compiler annotates only natural loops and may give this one two entries."""
    succ = {b["label"]: [t for t in b["succ"]] for b in bl if not b["top_header"]}
    for k in succ:
        succ[k] = [t for t in succ[k] if t in succ]
    index, low, stack, on, comps = {}, {}, [], set(), []
    for root in succ:   # Tarjan, iterative
        if root in index:
            continue
        work = [(root, iter(succ[root]))]
        index[root] = low[root] = len(index)
        stack.append(root)
        on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in index:
                    index[w] = low[w] = len(index)
                    stack.append(w)
                    on.add(w)
                    work.append((w, iter(succ[w])))
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == index[v]:
                    comp = set()
                    while True:
                        w = stack.pop()
                        on.discard(w)
                        comp.add(w)
                        if w == v:
                            break
                    comps.append(comp)
    holders = {b["label"] for b in bl if any("row_bcast" in i for i in b["ins"])}
    loops = [c for c in comps if len(c) > 1 and c & holders]
    if len(loops) != 1:
        raise SystemExit(f"expected one cycle with a row_bcast DPP step inside the item loop, found {len(loops)}")
    return min(loops[0]), [i for b in bl if b["label"] in loops[0] for i in b["ins"]]


def marked(lines, begin, end):
    """Instruction lines between each begin / end marker pair, in layout order."""
    regions, cur = [], None
    for l in lines:
        s = l.strip()
        if "PM_MARK " + begin in s:
            cur = []
        elif "PM_MARK " + end in s and cur is not None:
            regions.append(cur)
            cur = None
        elif cur is not None and l.startswith("\t") and not s.startswith(".") and not s.startswith(";"):
            cur.append(s)
    return regions


def marked_blocks(lines, begin, end):
    """Like marked(), but each region as its basic blocks in layout order: [label or None, instruction lines]."""
    regions, cur = [], None
    for l in lines:
        s = l.strip()
        if "PM_MARK " + begin in s:
            cur = [[None, []]]
        elif "PM_MARK " + end in s and cur is not None:
            regions.append(cur)
            cur = None
        elif cur is not None:
            m = re.match(r"\.L(BB\d+_\d+):", l)
            if m:
                cur.append([m.group(1), []])
            elif l.startswith("\t") and not s.startswith(".") and not s.startswith(";"):
                cur[-1][1].append(s)
    return regions


def full_row_path(region):
    """The instructions of the cheapest (fewest VALU) path from a slot region's first block to its end.  The region is
    forward-branching code; a full slot row skips the clamped-address DMA and the phantom-family selects, which are the
    only alternatives and both cost VALU instructions."""
    idx = {b[0]: i for i, b in enumerate(region) if b[0]}
    n = len(region)
    succ = []
    for i, (_, ins) in enumerate(region):
        s = [idx[m.group(1)] for x in ins for m in [re.match(r"s_c?branch\w*\s+\.L(BB\d+_\d+)", x)] if m and m.group(1) in idx]
        if not (ins and ins[-1].split()[0] == "s_branch"):
            s.append(i + 1)   # fall-through (n: the region's end)
        succ.append(s)
    cost = [sum(1 for x in ins if classify(x.split()[0], x) == "valu") for _, ins in region]
    best = [None] * (n + 1)
    best[n] = (0, [])
    for i in range(n - 1, -1, -1):
        c = [(best[j][0], j) for j in succ[i] if j > i and best[j] is not None]
        if c:
            w, j = min(c)
            best[i] = (cost[i] + w, [i] + best[j][1])
    return [x for i in best[0][1] for x in region[i][1]]


def slot_waits(path):
    """Every s_waitcnt lgkmcnt of a slot's executed path with what it retires.  LDS operations return in order, so
    lgkmcnt(n) retires all but the youngest n outstanding; with a scalar load outstanding (out of order) only
    lgkmcnt(0) retires anything for certain."""
    out, pending, valu = [], [], 0   # pending: (op, VALU count at its issue)
    for l in path:
        op = l.split()[0]
        c = classify(op, l)
        if c == "valu":
            valu += 1
        elif c in ("lds", "s_load"):
            pending.append((op, valu))
        elif c == "waitcnt_lgkm":
            n = int(re.search(r"lgkmcnt\((\d+)\)", l).group(1))
            smem = any(o.startswith("s_") for o, _ in pending)
            done = pending if n == 0 else ([] if smem else pending[:len(pending) - n] if n < len(pending) else [])
            pending = pending[len(done):]
            ring = [v for o, v in done if o.startswith("ds_read") and not o.startswith("ds_read_b64")]
            out.append({"lgkmcnt": n, "retires": len(done), "last": done[-1][0] if done else None,
                        "valu_gap": valu - done[-1][1] if done else None, "ring_gap": valu - ring[-1] if ring else None})
    return out


def account(targs, defines):
    plain_lines, res = kernel_lines(compile_asm(targs, defines))
    mark_lines, res_m = kernel_lines(compile_asm(targs, defines + ["PM_ISA_MARK=1"]))
    out = {"template_args": targs, "resources": res}
    bl = blocks(plain_lines)
    head, loop = brent_loop(bl)
    out["kernel"] = mix([i for b in bl for i in b["ins"]])
    out["brent_loop"] = mix(loop)
    out["brent_loop"]["s_load_lines"] = [i for i in loop if classify(i.split()[0], i) == "s_load"]
    out["brent_loop"]["valu_mov"] = sum(1 for i in loop if re.match(r"v_mov_b(32|64)(_e32|_e64)?\s", i))
    out["brent_loop"]["valu_cndmask"] = sum(1 for i in loop if i.startswith("v_cndmask"))
    blm = blocks(mark_lines)
    out["markers_neutral"] = (res == res_m and mix([i for b in blm for i in b["ins"]]) == out["kernel"]
                              and mix(brent_loop(blm)[1]) == {k: out["brent_loop"][k] for k in CLASSES})
    slots = [mix(r) for r in marked(mark_lines, "hoist_dn_slot_begin", "hoist_dn_slot_end")]
    if slots:
        out["hoist_slot"] = {"slots": len(slots), "valu_per_slot": [s["valu"] for s in slots],
                             "median": {k: statistics.median(s[k] for s in slots) for k in CLASSES}}
        paths = [full_row_path(r) for r in marked_blocks(mark_lines, "hoist_dn_slot_begin", "hoist_dn_slot_end")]
        out["hoist_slot"]["full_row"] = [{"valu": mix(p)["valu"], "s_load": mix(p)["s_load"], "lds": mix(p)["lds"],
                                          "lgkm_waits": slot_waits(p)} for p in paths]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("names", nargs="*", default=["headline", "plain128"])
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--label", default=None, help="key of this run in the --json file (default: the -D list, or 'default')")
    ap.add_argument("--json", default=None, help="merge the result into this JSON file under --label")
    a = ap.parse_args()
    result = {n: account(NAMES.get(n, n), a.defines) for n in a.names}
    for n, r in result.items():
        print(f"{n}: k_brent<{r['template_args']}>  {r['resources']}  markers_neutral={r['markers_neutral']}")
        for region in ("kernel", "brent_loop"):
            print(f"  {region:11s} " + "  ".join(f"{k}={r[region][k]}" for k in CLASSES))
        bl = r["brent_loop"]
        print(f"  brent_loop  v_mov={bl['valu_mov']}  v_cndmask={bl['valu_cndmask']}")
        for l in bl["s_load_lines"]:
            print(f"  brent_loop  {l}")
        if "hoist_slot" in r:
            print(f"  hoist_slot  x{r['hoist_slot']['slots']} median " + "  ".join(f"{k}={v}" for k, v in r["hoist_slot"]["median"].items()))
            for s, fr in enumerate(r["hoist_slot"]["full_row"]):
                waits = " ".join(f"lgkmcnt({w['lgkmcnt']})<-{w['last']}+{w['valu_gap']}v" for w in fr["lgkm_waits"][:3])
                more = len(fr["lgkm_waits"]) - 3
                print(f"  slot {s:2d} full row: valu={fr['valu']} s_load={fr['s_load']} lds={fr['lds']}  {waits}" + (f" (+{more} waits)" if more > 0 else ""))
    if a.json:
        label = a.label or (",".join(a.defines) if a.defines else "default")
        doc = json.load(open(a.json)) if os.path.exists(a.json) else {}
        doc.setdefault("mixes", {})[label] = result
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0 if all(r["markers_neutral"] for r in result.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
