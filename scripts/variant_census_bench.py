#!/usr/bin/env python3
"""Kernel time of the variant census (tps_batch_variant_census) beside the config-2 scan, on resident batches.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 scripts/variant_census_bench.py      # the workload
    scripts/variant_census_bench.py --check DIR/.../<pid>_kernel_trace.csv                               # time per launch and arm

The workload: 10 000 x 15 kb synthetic ONT reads per motif (the benchmark's config 2 shape) -- CCCTAA, AAACCCT and the 23-letter
C. albicans motif -- each batch resident in a slot of its own and scanned once with its default table (k = len - 2, window 100,
slide = len, the config-2 parameters; the 23-letter motif with --cutoff 0.1); the boundaries the scan calls give every read's tract, as `--variants` computes them.  Then,
alternating in one process and on one context:
  * the census of each batch against its motif (bin 500, 40 bins, with the profile), one launch per call;
  * the config-2 scan of the CCCTAA batch (bench.py's `value` region: step 1, windows, change point, sums stored), one launch per call.
No bar is set: nobody has measured this kernel before.  The kernels' times come from the profiler's dispatch timestamps (device
clocks); the launches of the census arms are told apart by their order, which the script fixes.  Without a profiler the script
prints the host's time per call (uploads of tails / begin / end, launch, kernel, outputs copied back, partial profiles added up) and,
for the scan, the library's own device-event time per launch."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CENSUS = "variant_census_kernel"
MOTIFS = [("CCCTAA", "CCCTAA"), ("AAACCCT", "AAACCCT"), ("albicans23", "ACGGATGTCTAACTTCTTGGTGT")]
CUTOFF = {"albicans23": 0.1}      # step 1's TRC cutoff where 0.7 (config 2) lets no read through: a 21-mer rarely survives ONT errors


def check(path, warmup):
    """Census dispatches in start order: launch i belongs to arm i mod 3 (after the 3 set-up launches main() makes, one per arm in
    the same order); the first `warmup` rounds are left out."""
    census, scans = [], []
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"].split("(")[0].strip()
            t = (int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]), name)
            if CENSUS in name:
                census.append(t)
            elif name.startswith("tps_scan_kernel"):
                scans.append(t)
    census.sort()
    scans.sort()
    out = dict(trace=path, census={}, scan={})
    for a, (name, unit) in enumerate(MOTIFS):
        d = [x[1] / 1000.0 for i, x in enumerate(census) if i % len(MOTIFS) == a and i // len(MOTIFS) >= 1 + warmup]
        if d:
            out["census"][name] = dict(unit_letters=len(unit), launches=len(d), median_us=round(statistics.median(d), 2), mean_us=round(statistics.fmean(d), 2),
                                       min_us=round(min(d), 2), max_us=round(max(d), 2))
    by_name = {}
    for _, d, name in scans:
        by_name.setdefault(name, []).append(d / 1000.0)
    for name, d in by_name.items():
        d = d[2 + warmup:] if len(d) > 2 + warmup else d      # (the config-2 kernel: two set-up scans and the warm-up rounds come first)
        out["scan"][name] = dict(launches=len(d), median_us=round(statistics.median(d), 2), mean_us=round(statistics.fmean(d), 2), min_us=round(min(d), 2), max_us=round(max(d), 2))
    print(json.dumps(out))
    return 0 if out["census"] else 2


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
    prms, tracts, totals = [], [], []
    for slot, (name, unit) in enumerate(MOTIFS):
        bases, offsets, _ = synth.make_reads(args.reads, args.len, unit, 20261019 + slot, errors=synth.ONT)
        sc.upload(slot, bases, offsets)
        pats = allsteps.patterns_to_search(telopattern=unit, cut_length=len(unit) - 2)
        no_bp = 1000
        prm = hiplib.make_params(no_bp=no_bp, min_len=9000, min_count=allsteps.min_count_for_cutoff(CUTOFF.get(name, 0.7), no_bp / len(unit), no_bp), window=100, slide=len(unit),
                                 trimfirst=100, maxlen=20000, jump=5, min_size=2, flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS)
        hiplib.set_table(sc, pats)
        sc.scan(slot, prm)
        sc.sync()
        res = sc.results(slot)
        hiplib.resolve_ties(sc, slot, res, len(pats), prm.jump, prm.min_size)
        begin, end = variants.tract_bounds(res, 100, len(unit), 20000)
        tails = np.where(end > begin, res["tail"], 0).astype(np.uint8)
        prms.append(prm)
        tracts.append((tails, begin, end))
    # (the set-up launches of the census, one per arm, in arm order: check() counts on it)
    for slot, (name, unit) in enumerate(MOTIFS):
        counts, profile = sc.variant_census(slot, unit, *tracts[slot])
        totals.append(counts.sum(axis=0, dtype=np.int64))
        assert np.array_equal(profile.sum(axis=0), totals[-1])
    hiplib.set_table(sc, allsteps.patterns_to_search(telopattern="CCCTAA", cut_length=4))
    sc.scan(0, prms[0])
    sc.sync()
    sc.kernel_time_reset()

    def scan():
        sc.scan(0, prms[0])
        sc.sync()
    arms = {name: (lambda s=slot, u=unit: sc.variant_census(s, u, *tracts[s])) for slot, (name, unit) in enumerate(MOTIFS)}
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
                  host_ms_per_call={name: round(1000.0 * statistics.median(s), 3) for name, s in spent.items()}, tracts={})
    for (name, unit), (tails, begin, end), tot in zip(MOTIFS, tracts, totals):
        n, canon, other, cls = variants.split_row(tot, unit)
        report["tracts"][name] = dict(reads_with_tract=int((end > begin).sum()), positions=n, canonical_share=round(canon / max(n, 1), 4),
                                      variant_share=round(sum(cls) / max(n, 1), 4), other_share=round(other / max(n, 1), 4))
    print(json.dumps(report))
    sc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
