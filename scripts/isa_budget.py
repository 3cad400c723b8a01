#!/usr/bin/env python3
"""Static per-phase instruction budget of one scan kernel (no GPU needed).

Compiles the kernel's group with -DTPS_ISA_MARKS (the clock-stamp boundaries and the phases of the sums tiles become
comments in the ISA, nothing else: csrc/tps_wave.h, TPS_ISA_MARK) and counts the instructions between consecutive marks
in the kernel's text, in layout order: VALU (v_*), LDS (ds_*), VMEM (global_*, buffer_*), SALU (s_*, without s_waitcnt,
s_nop, branches and barriers).  Static counts: a loop body counts once, a branch's both sides count.

  usage: scripts/isa_budget.py [--kernel tps_scan_kernel_s6p] [--group 1] [--src DIR] [--csv OUT]

--src: the csrc directory of another copy of the tree to compile instead of this one's (e.g. an older revision, for a
before/after; scripts/isa_diff.py shows how to take one from git).
Rows: the kernel's regions between clock stamps (step 1 = stamps 1..4, the change point = 9..10), and per tile
instantiation (S, RPT, ROTZ, PAIR) its phases; `home` marks the instantiation of the default geometry (slide 6, r = 0,
q a multiple of 8, pair table), the one config 2 runs five times per read.  The strided candidate pass is a loop (config 2:
two passes per tile) that a tile which stores its candidates lane by lane skips.  `region*` rows are the parts of a read's
program outside the tile phases (TPS_ISA_REGION): tile set-up, per tile the staging store, the prefetch and the dispatch,
the change point's stages, and step 1 of the pair-table kernels (trc_decide_pairs: the static rows `stamp2` / `stamp3` behind
it are the older routes, which such a kernel keeps for dirty heads and heads over the bound); REGION_LOWER holds a written
floor for each."""
import argparse
import csv
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASES = {1: "phase1_blocks", 2: "windows", 3: "scan_store_prefix_lanecands", 4: "gsum", 6: "strided_candidates", 5: "tile_end"}
STAMPS = {0: "entry", 1: "step1_stage_count", 2: "step1_decide", 3: "step1_decide", 4: "tiles_setup", 5: "tile_loop",
          6: "tile_loop", 7: "tile_loop", 8: "tile_loop", 9: "change_point", 10: "results"}
# a written lower bound per tile-lane phase of the home instantiation (slide 6, pair table, 8 blocks, 8 windows per lane):
# phase 1: 24 pair lookups (an address each) + 8 block ORs and count adds; windows: per window a 3-input NOR and a popcount,
# per window pair one packed subtract + add of the counts; scan: 6 DPP steps and 8 prefix adds; candidates: the lane's first
# candidate (window address, magic division: add, mulhi) and its window (mul, sub), the second one's window and whether it is
# the lane's own (add, compare, two selects), two row addresses, two sums, two store offsets = 15
# (the strided pass: none -- the lanes' own candidates need no second pass)
LOWER = {1: 24 + 16, 2: 8 * 2 + 4 * 2, 3: 6 + 8 + 15, 4: 2, 6: 0, 5: 0}
REGIONS = {1: "tile_setup", 2: "stage_store", 3: "prefetch", 4: "tile_dispatch", 5: "binseg_prefilter", 6: "binseg_f64_reduce",
           7: "binseg_exact_result", 8: "binseg_one_lane", 9: "step1_pairs"}
# written floors of the regions, VALU per wave and execution (static rows hold BOTH sides of every branch, so a row can lie
# above its floor by the side a read does not take):
# 1 tile set-up: the first prefetch (a lane id, a compare, four zeros) -- everything else is wave-uniform: 6
# 2 staging store, one quad per lane: an LDS address and the compare against the buffer's quads, + the reversal of a reverse
#   tail (4 words x bfrev, two shifts, bfi): 2 forward, 18 reverse
# 3 prefetch: the compare against the staged quads and four zeros under the masked load; the address is per read: 5
# 4 dispatch: the invalid flag's LDS read and its readfirstlane; the switch is scalar: 2
# 5 prefilter, integer route, per candidate of a full group: D (24-bit multiply-add, its addend's step, cvt), the denominator
#   (b's step, subtract, multiply), rcp, two multiplies, compare + med3 + three selects for best / runner-up = 14, 56 per group;
#   the group that holds the last used slot adds an offset, a clamp, a compare and a select per candidate: 72; + per read the
#   lane's first candidate (index, offset, b, -T b: 6), its index rebuilt from the slot (3), the wave maximum (6 DPP steps, a
#   readlane), the threshold and the two ballots' compares: 20.  Static rows hold four groups of both kinds and the four checked
#   groups of the float64 route; a config-2 read runs one full and one checked group: 56 + 72 + 20 = 148
# 8 one-lane finish: two readlanes, D (2 cvt, mul, fma), numerator and denominator (3), three float64 divisions (the score
#   and the gain's two, about 11 each): 42
# 6 one float64 candidate per lane (41, the fraction comparison as written) + one division (about 12) + three wave maxima
#   (21) + two ballots' compares: 76 -- only reads with two or more close lanes, a crowded lane or no prefilter come here
# 7 the exact tournament never runs without a tie; the gain's two divisions are counted with the finish that ran: 0
# 9 step 1 of the pair-table kernels (trc_decide_pairs), a table of at most 12 patterns: the lane's bit offset and word index (3),
#   three funnel shifts of its bases, 16 pair lookups (a v_alignbit except at the two register boundaries, a v_and: 30), the
#   carry-save adders (12 full adders of two v_bitop3, 2 half adders, one OR: 29), the fix-up lookup behind its lane compare
#   (offset, index, funnel shift, v_and + v_or of the single table's base: 6) and the full lanes' compare; planes to bytes for
#   three words (per word 4 x field, multiply, mask, and 3 merges: 15, 45), three row sums of 5 DPP adds and 2 readlanes (21):
#   138.  The arg-max is scalar.  The counts' store (only when the caller asks for them: the lane's pattern and side, two 4-way
#   word selects, shift, mask, address) is another 36 in the static row, and the fourth word (P > 12) another 15 + 7
REGION_LOWER = {1: 6, 2: 2, 3: 5, 4: 2, 5: 56 + 72 + 20, 6: 76, 7: 0, 8: 42, 9: 138}


def compile_isa(src, group, out):
    hipcc = "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-fno-vectorize", "-std=c++17", "-fPIC", "-Wno-unused-variable",
           "-DTPS_ISA_MARKS", f"-DTPS_KGROUP={group}", "-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
           "-o", out, os.path.join(src, "tps_kernels.hip" if group else "topsicle_hip.hip")]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)


def kind(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    if op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_barrier", "s_endpgm")):
        return "salu"
    return None


def regions(isa_path, kernel):
    lines = open(isa_path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(kernel + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end") or lines[i].startswith(".Lfunc_end"))
    acc, cur = {}, ("stamp", 0)
    for l in lines[start + 1:end]:
        m = re.search(r";tps_(stamp|mark|region) (0x[0-9a-f]+|\d+)", l)
        if m:
            cur = (m.group(1), int(m.group(2), 0))
            continue
        t = l.strip()
        if not t or t.startswith((";", ".", "//")):
            continue
        k = kind(t.split()[0])
        if k:
            d = acc.setdefault(cur, {"valu": 0, "lds": 0, "vmem": 0, "salu": 0})
            d[k] += 1
    return acc


def decode(mk):
    p = mk % 10
    S = (mk // 10) % 100
    rpt = (mk // 1000) % 100 - 1
    rotz, pair, inv, cd = (mk // 100000) % 10, (mk // 1000000) % 10, (mk // 10000000) % 10, (mk // 100000000) % 10
    return p, S, rpt, rotz, pair, inv, cd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="tps_scan_kernel_s6p")
    ap.add_argument("--group", type=int, default=1)
    ap.add_argument("--src", default=os.path.join(ROOT, "topsicle_amd", "csrc"))
    ap.add_argument("--csv", default="")
    ap.add_argument("--tag", default="")
    o = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        isa = os.path.join(td, "k.s")
        compile_isa(o.src, o.group, isa)
        acc = regions(isa, o.kernel)
    rows = []
    for (what, v), d in sorted(acc.items()):
        if what == "stamp":
            rows.append(dict(tag=o.tag, kernel=o.kernel, region=f"stamp{v}_{STAMPS.get(v, '?')}", S="", rpt="", rotz="", pair="", home="",
                             lower_bound_valu="", **d))
        elif what == "region":
            rows.append(dict(tag=o.tag, kernel=o.kernel, region=f"region{v}_{REGIONS.get(v, '?')}", S="", rpt="", rotz="", pair="", home="",
                             lower_bound_valu=REGION_LOWER.get(v, ""), **d))
        else:
            p, S, rpt, rotz, pair, inv, cd = decode(v)
            home = int(S == 6 and rpt == 0 and rotz == 1 and pair == 1 and inv == 0 and cd == 0)
            rows.append(dict(tag=o.tag, kernel=o.kernel, region=f"tile_{PHASES[p]}", S=S, rpt=rpt, rotz=rotz, pair=pair, home=home,
                             lower_bound_valu=LOWER[p] if home else "", **d))
    cols = ["tag", "kernel", "region", "S", "rpt", "rotz", "pair", "home", "valu", "lds", "vmem", "salu", "lower_bound_valu"]
    w = csv.DictWriter(open(o.csv, "a" if os.path.exists(o.csv) else "w", newline="") if o.csv else sys.stdout, fieldnames=cols)
    if not o.csv or os.path.getsize(o.csv) == 0:
        w.writeheader()
    for r in rows:
        w.writerow({k: r.get(k, "") for k in cols})
    home = [r for r in rows if r["home"] == 1]
    print(f"# {o.tag} {o.kernel}: home tile VALU per tile-lane (static) = {sum(r['valu'] for r in home)}", file=sys.stderr)


if __name__ == "__main__":
    main()
