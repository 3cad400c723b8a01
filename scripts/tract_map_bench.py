#!/usr/bin/env python3
"""Kernel time of the tract map (tps_batch_tract_map) beside the config-2 scan and the variant census, on resident batches.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 scripts/tract_map_bench.py      # the workload
    scripts/tract_map_bench.py --check DIR/.../<pid>_kernel_trace.csv                               # time per launch and arm

The workload: 10 000 x 15 kb synthetic ONT reads per motif (the benchmark's config 2 shape) -- CCCTAA and the 23-letter C. albicans
motif -- each batch resident in a slot of its own.  Alternating in one process and on one context:
  * the map of each batch against its motif with the defaults (block 64, min_hits 20, gap 1, min_blocks 2, 8 tracts), one launch per call;
  * the variant census of the CCCTAA batch's called tracts (bin 500, 40 bins), one launch per call;
  * the config-2 scan of the CCCTAA batch (bench.py's `value` region: step 1, windows, change point, sums stored), one launch per call.
No bar is set: nobody has measured this kernel before.  The kernels' times come from the profiler's dispatch timestamps (device
clocks); the launches of the two map arms are told apart by their order, which the script fixes.  Without a profiler the script prints
the host's time per call (table built and uploaded, launch, kernel, outputs copied back) and, for the scan, the library's own
device-event time per launch."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MOTIFS = [("CCCTAA", "CCCTAA"), ("albicans23", "ACGGATGTCTAACTTCTTGGTGT")]


def _stats(d):
    return dict(launches=len(d), median_us=round(statistics.median(d), 2), mean_us=round(statistics.fmean(d), 2), min_us=round(min(d), 2), max_us=round(max(d), 2))


def check(path, warmup):
    """Map dispatches in start order: launch i belongs to arm i mod 2 (after the 2 set-up launches main() makes, one per arm in the
    same order); the first `warmup` rounds are left out."""
    maps, census, scans = [], [], {}
    with open(path, newline="") as fh:
        for row in sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"])):
            name = row["Kernel_Name"].split("(")[0].strip()
            d = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0
            if "tract_map_kernel" in name:
                maps.append(d)
            elif "variant_census_kernel" in name:
                census.append(d)
            elif name.startswith("tps_scan_kernel"):
                scans.setdefault(name, []).append(d)
    out = dict(trace=path, tract_map={}, variant_census={}, scan={})
    for a, (name, unit) in enumerate(MOTIFS):
        d = [x for i, x in enumerate(maps) if i % len(MOTIFS) == a and i // len(MOTIFS) >= 1 + warmup]
        if d:
            out["tract_map"][name] = dict(unit_letters=len(unit), **_stats(d))
    if len(census) > 1 + warmup:
        out["variant_census"]["CCCTAA"] = _stats(census[1 + warmup:])
    for name, d in scans.items():
        out["scan"][name] = _stats(d[2 + warmup:] if len(d) > 2 + warmup else d)      # (two set-up scans and the warm-up rounds come first)
    print(json.dumps(out))
    return 0 if out["tract_map"] else 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", help="a kernel_trace.csv of rocprofv3 --kernel-trace: print the time per launch of every arm")
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--len", type=int, default=15000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.check:
        return check(args.check, args.warmup)
    import numpy as np
    from topsicle_amd import allsteps, hiplib, synth, variants
    sc = hiplib.HipScanner(0)
    found = {}
    for slot, (name, unit) in enumerate(MOTIFS):
        bases, offsets, _ = synth.make_reads(args.reads, args.len, unit, 20261019 + slot, errors=synth.ONT)
        sc.upload(slot, bases, offsets)
    # (the set-up launches of the map, one per arm, in arm order: check() counts on it)
    for slot, (name, unit) in enumerate(MOTIFS):
        t, f, totals = sc.tract_map(slot, unit)
        found[name] = dict(reads_with_one_tract=int((f.sum(axis=1) == 1).sum()), reads_without=int((f.sum(axis=1) == 0).sum()),
                           hits_per_read=round(float(totals[:, :2].sum(axis=1).mean()), 1))
    no_bp, unit = 1000, "CCCTAA"
    pats = allsteps.patterns_to_search(telopattern=unit, cut_length=4)
    prm = hiplib.make_params(no_bp=no_bp, min_len=9000, min_count=allsteps.min_count_for_cutoff(0.7, no_bp / len(unit), no_bp), window=100, slide=len(unit),
                             trimfirst=100, maxlen=20000, jump=5, min_size=2, flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS)
    hiplib.set_table(sc, pats)
    for _ in range(2):
        sc.scan(0, prm)
        sc.sync()
    res = sc.results(0)
    hiplib.resolve_ties(sc, 0, res, len(pats), prm.jump, prm.min_size)
    begin, end = variants.tract_bounds(res, 100, len(unit), 20000)
    tails = np.where(end > begin, res["tail"], 0).astype(np.uint8)
    sc.variant_census(0, unit, tails, begin, end)

    def scan():
        sc.scan(0, prm)
        sc.sync()
    arms = {"tract_map_" + name: (lambda s=slot, u=u: sc.tract_map(s, u)) for slot, (name, u) in enumerate(MOTIFS)}
    arms["variant_census_CCCTAA"] = lambda: sc.variant_census(0, unit, tails, begin, end)
    arms["config2_scan"] = scan
    spent = {name: [] for name in arms}
    for i in range(args.warmup + args.calls):
        if i == args.warmup:
            sc.kernel_time_reset()
        for name, call in arms.items():
            t0 = time.perf_counter()
            call()
            if i >= args.warmup:
                spent[name].append(time.perf_counter() - t0)
    n_launches, total_ms, mean_ms = sc.kernel_time_ms()
    report = dict(reads=args.reads, read_len=args.len, calls=args.calls, device=sc.device_info(), scan_kernel=sc.kernel_info(0),
                  scan_event_us_per_launch=round(1000.0 * mean_ms, 2), scan_event_launches=n_launches,
                  host_ms_per_call={name: round(1000.0 * statistics.median(s), 3) for name, s in spent.items()}, maps=found)
    print(json.dumps(report))
    sc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
