#!/usr/bin/env python3
"""Kernel time of the base-modification profile (tps_batch_mod_profile) beside the config-2 scan and the refined boundary, on one
resident batch.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/methyl_bench.py       # the workload
    scripts/methyl_bench.py --check DIR/.../<pid>_kernel_trace.csv                                        # time per launch

The workload: 10 000 x 15 kb synthetic ONT reads (the benchmark's config 2 shape), resident in one slot and scanned once with the
config-2 parameters; every read carries one entry per CpG of its sequence (what a 5mC model emits for a C+m? tag) and is profiled over
the default region, [boundary - 2 x 500, boundary + 8 x 500), around the boundary the scan called -- or around 3000 where it called
none, so that every read does the same work.  Then, alternating in one process and on one context: the profile, the refined boundary
of the same batch (tps_batch_boundary_refine against CCCTAA over [100, 15000)), and the config-2 scan (bench.py's `value` region).
No bar is set: nobody has measured this kernel before.  The kernels' times come from the profiler's dispatch timestamps (device
clocks).  Without a profiler the script prints the host's time per call and the bytes a call takes up."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("mod_profile_kernel", "boundary_refine_kernel", "tps_scan_kernel")


def check(path, warmup):
    """Time per launch of every kernel of KERNELS, the set-up launch and the first `warmup` rounds left out."""
    seen = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"].split("(")[0].strip()
            key = next((k for k in KERNELS if k in name), None)
            if key is not None:
                seen.setdefault(name, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    out = dict(trace=path, kernels={})
    for name, ts in seen.items():
        d = [x[1] / 1000.0 for x in sorted(ts)]
        d = d[1 + warmup:] if len(d) > 1 + warmup else d
        out["kernels"][name] = dict(launches=len(d), median_us=round(statistics.median(d), 2), mean_us=round(statistics.fmean(d), 2), min_us=round(min(d), 2),
                                    max_us=round(max(d), 2))
    print(json.dumps(out))
    return 0 if any("mod_profile_kernel" in k for k in out["kernels"]) else 2


def cpg_entries(bases, offsets):
    """(mod_off, delta, prob): one entry on every C that a G follows, per read -- positions to skip counts among the read's C's."""
    import numpy as np
    is_c = (bases == ord("C"))
    nxt = np.zeros(len(bases), bool)
    nxt[:-1] = bases[1:] == ord("G")
    nxt[offsets[1:] - 1] = False                   # (a read's last base has none behind it)
    rank = np.cumsum(is_c) - 1                     # ordinal of every C over the whole batch
    site = np.nonzero(is_c & nxt)[0]
    read_of = np.searchsorted(offsets, site, side="right") - 1
    c_before = np.concatenate(([0], np.cumsum(is_c)))[offsets[:-1]]
    ordinal = rank[site] - c_before[read_of]
    first = np.ones(len(site), bool)
    first[1:] = read_of[1:] != read_of[:-1]
    delta = np.where(first, ordinal, ordinal - np.concatenate(([0], ordinal[:-1])) - 1)
    mod_off = np.searchsorted(read_of, np.arange(len(offsets)), side="left").astype(np.int64)
    prob = ((site * 2654435761) >> 7).astype(np.uint8)
    return mod_off, delta.astype(np.uint32), prob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", help="a kernel_trace.csv of rocprofv3 --kernel-trace: print the time per launch of every kernel")
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--len", type=int, default=15000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.check:
        return check(args.check, args.warmup)
    import numpy as np
    from topsicle_amd import allsteps, hiplib, methyl, refine, synth, variants
    sc = hiplib.HipScanner(0)
    unit = "CCCTAA"
    bases, offsets, _ = synth.make_reads(args.reads, args.len, unit, 20261021, errors=synth.ONT)
    sc.upload(0, bases, offsets)
    no_bp = 1000
    prm = hiplib.make_params(no_bp=no_bp, min_len=9000, min_count=allsteps.min_count_for_cutoff(0.7, no_bp / len(unit), no_bp), window=100, slide=6,
                             trimfirst=100, maxlen=20000, jump=5, min_size=2, flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS)
    pats = allsteps.patterns_to_search(telopattern=unit, cut_length=4)
    hiplib.set_table(sc, pats)
    sc.scan(0, prm)
    sc.sync()
    res = sc.results(0)
    hiplib.resolve_ties(sc, 0, res, len(pats), prm.jump, prm.min_size)
    n = args.reads
    tails = res["tail"].astype(np.uint8)
    spec = methyl.MethylSpec()
    boundary = variants.tract_bounds(res, 100, 6, 20000)[1]
    origin = np.where(boundary > 0, boundary, 3000).astype(np.int32)
    begin = np.maximum(0, origin - spec.nb0 * spec.w).astype(np.int32)
    end = (origin + spec.nb1 * spec.w).astype(np.int32)
    mod_off, delta, prob = cpg_entries(np.asarray(bases), np.asarray(offsets))
    r_begin, r_end = np.full(n, 100, np.int32), np.full(n, 15000, np.int32)
    at = refine.regions(res, 100, 6, 20000, 6)[2]

    def scan():
        sc.scan(0, prm)
        sc.sync()
    arms = {"mod_profile": lambda: sc.mod_profile(0, tails, begin, end, origin, mod_off, delta, prob, w=spec.w, nb0=spec.nb0, nb1=spec.nb1, hi=spec.hi, lo=spec.lo),
            "boundary_refine": lambda: sc.boundary_refine(0, unit, tails, r_begin, r_end, at),
            "config2_scan": scan}
    rows, bins = arms["mod_profile"]()             # (the set-up launch: check() leaves it out)
    first = dict(entries=int(rows["entries"].sum()), in_region=int(rows["in_region"].sum()), called=int(rows["called"].sum()), cpg=int(rows["cpg"].sum()),
                 off_context=int(rows["off_context"].sum()), bad=int((rows["flags"] != 0).sum()), high=int(bins["high"].sum()), low=int(bins["low"].sum()))
    assert first["bad"] == 0 and first["off_context"] == 0 and first["called"] == first["cpg"] == first["in_region"]      # an entry on every CpG, and on nothing else
    arms["boundary_refine"]()
    spent = {name: [] for name in arms}
    for i in range(args.warmup + args.calls):
        for name, call in arms.items():
            t0 = time.perf_counter()
            call()
            if i >= args.warmup:
                spent[name].append(time.perf_counter() - t0)
    up = dict(regions=int(n * 13), mod_off=int(8 * (n + 1)), delta=int(4 * len(delta)), prob=int(len(prob)))
    print(json.dumps(dict(reads=args.reads, read_len=args.len, bins=[spec.nb0, spec.nb1, spec.w], calls=args.calls, device=sc.device_info(), scan_kernel=sc.kernel_info(0),
                          first_call=first, bytes_up_per_call=dict(up, total=sum(up.values())), bytes_down_per_call=int(rows.nbytes + bins.nbytes),
                          host_ms_per_call={name: round(1000.0 * statistics.median(s), 3) for name, s in spent.items()})))
    sc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
