#!/usr/bin/env python3
"""Static instruction census of one instantiation of the wave kernel (csrc/bdx_wave_kernel.h, as csrc/bdx_wave.hip
or another of its translation units instantiates it: --src), read from its gfx950 assembly.

    python tools/wave_isa_census.py                      # the headline form, compiled from the tree (~2 min, CPU only)
    python tools/wave_isa_census.py --asm wave.s         # an assembly file kept from an earlier run (--keep wave.s)
    python tools/wave_isa_census.py --inst 32,12,5,8,false,0,0,false,0,false,false

Prints the resource lines (VGPRs, SGPRs, scratch), the loops of the function (found from the backward branches), the
static v_readlane / v_writelane inside the per-tile loop (all of them, and those on the registers the compiler spills
SGPRs into: the VGPRs some v_writelane writes), and the VALU counts of the seed scan's round loop (the trips of a round
are unrolled in it: five in the headline form, one round per tile), of the loops nested in it (the hit append, once per
round) and of the first sweep loop.  Per loop, and for the tile loop's own body, it also counts the cheap-class VALU
instructions (v_and / or / xor / add / sub / lshrrev) that take a scalar register or a 32-bit literal as a source: the dearer
operand classes of tools/ubench_ops.hip (columns +sgpr, +lit).  Static counts: what one pass through a loop's body issues; how often each body runs
depends on the data (the per-round lines show it for L layers / hits of the fullest lane over the round).
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "biodemux.jl_amd", "csrc")
HEADLINE = "32,20,5,8,false,0,0,false,0,false,false"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only", "-S"]


def mangle(inst: str) -> str:
    out = []
    for v in inst.split(","):
        v = v.strip()
        out.append("Lb1E" if v == "true" else "Lb0E" if v == "false" else "Li%dE" % int(v))
    return "_ZN12_GLOBAL__N_115bdx_wave_kernelI" + "".join(out) + "EEvNS_8WaveArgsE"


def compile_asm(src: str, keep: str | None) -> str:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = keep or os.path.join(tempfile.mkdtemp(prefix="wave_census_"), "bdx_wave.s")
    subprocess.check_call([hipcc, *FLAGS, src, "-o", out], cwd=os.path.dirname(src))
    return out


def function_body(asm: str, name: str):
    lines = asm.split("\n")
    st = next((i for i, l in enumerate(lines) if l.startswith(name + ":")), None)
    if st is None:
        sys.exit("instantiation not in the assembly: " + name)
    en = next(i for i in range(st, len(lines)) if lines[i].startswith(".Lfunc_end"))
    tail = lines[en:en + 60]
    res = {}
    for l in tail:
        m = re.match(r";\s*(TotalNumSgprs|NumVgprs|TotalNumVgprs|ScratchSize|Occupancy):\s*(\d+)", l)
        if m:
            res[m.group(1)] = int(m.group(2))
    return lines[st:en], res


def is_valu(l: str) -> bool:
    return re.match(r"\s+v_", l) is not None


def is_salu(l: str) -> bool:
    return re.match(r"\s+s_(?!waitcnt|nop|branch|cbranch|setprio|barrier|sleep)", l) is not None


# The cheap class of tools/ubench_ops.hip: 2.4 clk with vector-register operands, 3.5 with a literal, 4.3 with a scalar register
CHEAP = ("v_and_b32", "v_or_b32", "v_xor_b32", "v_add_u32", "v_sub_u32", "v_subrev_u32", "v_lshrrev_b32")


def dear_operand(l: str):
    """"sgpr" / "lit" if the line is a cheap-class VALU instruction with a scalar-register or a 32-bit literal source operand
    (inline constants -16 .. 64 are neither), else None."""
    m = re.match(r"\s+(v_\w+?)(?:_e32|_e64)?\s+(.*)", l)
    if not m or m.group(1) not in CHEAP:
        return None
    kind = None
    for op in m.group(2).split(";")[0].split(",")[1:]:
        op = op.strip()
        if re.match(r"(s\d+|s\[|vcc|exec|ttmp|m0)", op):
            return "sgpr"
        if re.match(r"-?(0x[0-9a-fA-F]+|\d+)$", op) and not -16 <= int(op, 0) <= 64:
            kind = "lit"
    return kind


def count_dear(body, a, b, skip=()):
    """(cheap-class VALU with a scalar-register operand, with a literal operand) of lines a..b, without the ranges in skip."""
    s = t = 0
    for i in range(a, b + 1):
        if any(x <= i <= y for x, y in skip):
            continue
        k = dear_operand(body[i])
        s += k == "sgpr"
        t += k == "lit"
    return s, t


def loops(body):
    """(header line, last back-edge line, label) per loop header: the union of its back-edges."""
    lab = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            lab[m.group(1)] = i
    ends = {}
    for i, l in enumerate(body):
        m = re.match(r"\s+s_(?:cbranch_\w+|branch)\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in lab and lab[m.group(1)] < i:
            h = lab[m.group(1)]
            ends[h] = max(ends.get(h, 0), i)
    return sorted((h, e, body[h].split(":")[0]) for h, e in ends.items())


def count(body, a, b, skip=()):
    """VALU / SALU / LDS instructions of lines a..b, without the ranges in skip."""
    v = s = d = 0
    for i in range(a, b + 1):
        if any(x <= i <= y for x, y in skip):
            continue
        l = body[i]
        v += is_valu(l)
        s += is_salu(l)
        d += re.match(r"\s+ds_", l) is not None
    return v, s, d


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--inst", default=HEADLINE, help="template arguments of bdx_wave_kernel (default: the headline form)")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--src", default=os.path.join(CSRC, "bdx_wave.hip"), help="translation unit to compile")
    ap.add_argument("--keep", help="write the compiled assembly here")
    args = ap.parse_args()

    asm_path = args.asm or compile_asm(args.src, args.keep)
    body, res = function_body(open(asm_path).read(), mangle(args.inst))
    print("instantiation  bdx_wave_kernel<%s>" % args.inst)
    print("resources      VGPRs %s  SGPRs %s  scratch %s  occupancy %s" % (res.get("NumVgprs"), res.get("TotalNumSgprs"),
                                                                           res.get("ScratchSize"), res.get("Occupancy")))
    lp = loops(body)
    if not lp:
        sys.exit("no loops found")
    tile = max(lp, key=lambda x: x[1] - x[0])
    spill_v = set(re.findall(r"v_writelane_b32\s+(v\d+)", "\n".join(body)))
    rw_all = [i for i in range(tile[0], tile[1] + 1) if re.match(r"\s+v_(readlane|writelane)_b32", body[i])]
    def lane_vgpr(l):  # v_readlane_b32 sD, vS, lane / v_writelane_b32 vD, sS, lane
        m = re.search(r"v_readlane_b32\s+\S+,\s*(v\d+)", l) or re.search(r"v_writelane_b32\s+(v\d+)", l)
        return m.group(1) if m else None
    rw_spill = [i for i in rw_all if lane_vgpr(body[i]) in spill_v]
    total_rw = sum(1 for l in body if re.match(r"\s+v_(readlane|writelane)_b32", l))
    print("readlane/writelane  function %d, tile loop %d (on spill VGPRs %s: %d)" % (total_rw, len(rw_all), ",".join(sorted(spill_v)) or "none", len(rw_spill)))

    # the seed scan's round loop and its hit append: the append's write loop is the first innermost loop with a v_ffbl_b32 and
    # an LDS write; the round is the smallest loop around it that also holds the bitmap probes (sixteen per unrolled trip); the
    # loops in the round with a v_mbcnt or that write loop are the append's per-layer loops (they run once per layer: L = hits
    # of the fullest lane over the round)
    inner = [x for x in lp if tile[0] <= x[0] and x[1] <= tile[1] and x != tile]
    def nested(o):
        return [x for x in inner if o[0] <= x[0] and x[1] <= o[1] and x != o]
    def has(x, pat):
        return sum(1 for i in range(x[0], x[1] + 1) if re.search(pat, body[i]))
    writes = [x for x in inner if has(x, r"v_ffbl_b32") and has(x, r"ds_write") and not nested(x)]
    wr = min(writes) if writes else None
    trips = [x for x in inner if wr and wr in nested(x) and has(x, r"ds_read_b32") >= 16]
    trip = min(trips, key=lambda x: x[1] - x[0]) if trips else None
    layer = [x for x in nested(trip) if not nested(x) and (x == wr or has(x, r"v_mbcnt_lo"))] if trip else []
    print()
    # +sgpr / +lit: cheap-class VALU (v_and / or / xor / add / sub / lshrrev) of the loop's own body with a scalar-register / a
    # 32-bit literal source operand — the dearer operand classes of tools/ubench_ops.hip
    print("%-12s %13s  %5s %5s %4s %5s %4s" % ("loop", "lines", "VALU", "SALU", "LDS", "+sgpr", "+lit"))
    for x in inner:
        depth = sum(1 for y in inner if y[0] <= x[0] and x[1] <= y[1] and y != x)
        skip = [(y[0], y[1]) for y in nested(x)]
        v, s_, d = count(body, x[0], x[1], skip)
        ds, dl = count_dear(body, x[0], x[1], skip)
        tag = "scan round" if x == trip else ("append, per layer" if x in layer else "")
        print("%-12s %6d-%-6d  %5d %5d %4d %5d %4d  %s%s" % (x[2], x[0], x[1], v, s_, d, ds, dl, "  " * depth, tag))
    # the tile loop's own body (transcode, per-tile tables, verdicts: everything outside the loops above)
    ds, dl = count_dear(body, tile[0], tile[1], [(y[0], y[1]) for y in nested(tile)])
    v, s_, d = count(body, tile[0], tile[1], [(y[0], y[1]) for y in nested(tile)])
    print("%-12s %6d-%-6d  %5d %5d %4d %5d %4d  tile loop, own body" % (tile[2], tile[0], tile[1], v, s_, d, ds, dl))
    if trip:
        tv, ts, _ = count(body, trip[0], trip[1], [(y[0], y[1]) for y in layer])
        per = [count(body, y[0], y[1]) for y in layer]
        lv, ls = sum(v for v, _, _ in per), sum(s_ for _, s_, _ in per)
        print()
        ntrips = has(trip, r"ds_read_b32") // 16
        print("scan round %s (%d trips unrolled: %d probes) without the per-layer append loops: VALU %d, SALU %d" % (trip[2], ntrips, 16 * ntrips, tv, ts))
        for y, (v, s_, _) in zip(layer, per):
            print("append loop %s: VALU %d, SALU %d per layer" % (y[2], v, s_))
        for L in (1, 3, 5, 7):
            print("round with hits, L = %d layers: %d + %d = %d VALU, %d + %d SALU" % (L, tv, L * lv, tv + L * lv, ts, L * ls))
    sweeps = [x for x in inner if count(body, x[0], x[1])[0] > 300 and (not trip or x[0] > trip[1])]
    if sweeps:
        sw = min(sweeps, key=lambda x: (x[0], x[1] - x[0]))
        sw = min((x for x in sweeps if x[0] == sweeps[0][0]), key=lambda x: x[1] - x[0])
        v, s, d = count(body, sw[0], sw[1])
        print("first sweep loop %s (lines %d-%d, nested loops included): VALU %d, SALU %d, LDS %d" % (sw[2], sw[0], sw[1], v, s, d))


if __name__ == "__main__":
    main()
