#!/usr/bin/env python3
"""Kernel time of the boundary refinement (tps_batch_boundary_refine) beside the config-2 scan and the tract map, on one resident batch.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/refine_bench.py       # the workload
    scripts/refine_bench.py --check DIR/.../<pid>_kernel_trace.csv                                        # time per launch and arm

The workload: 10 000 x 15 kb synthetic ONT reads (the benchmark's config 2 shape), resident in one slot and scanned once with the
config-2 parameters; every read is refined over the region [100, 15000) on the tail the scan gave it (every read, not only those with
a stored boundary: the kernel's time does not depend on what the region holds), with the called boundary as `at`.  Then, alternating
in one process and on one context:
  * the refinement against CCCTAA and against the 23-letter C. albicans motif (w = 6 and w = 8: a table of 1 KB and of 16 KB), one
    launch per call (two arms);
  * the tract map of the same batch against CCCTAA (the defaults), which stages the same bases and does the same lookup for two strands;
  * the config-2 scan (bench.py's `value` region: step 1, windows, change point, sums stored).
No bar is set: nobody has measured this kernel before.  The kernels' times come from the profiler's dispatch timestamps (device
clocks); the launches of the two refinement arms are told apart by their order, which the script fixes.  Without a profiler the script
prints the host's time per call."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNEL = "boundary_refine_kernel"
ARMS = [("CCCTAA", "CCCTAA"), ("albicans23", "ACGGATGTCTAACTTCTTGGTGT")]
REGION = (100, 15000)


def check(path, warmup):
    """Refinement dispatches in start order: launch i belongs to arm i mod 2 (after the set-up round main() makes, one launch per arm
    in the same order); the first `warmup` rounds are left out."""
    ours, others = [], {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"].split("(")[0].strip()
            t = (int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
            if KERNEL in name:
                ours.append(t)
            elif name.startswith("tps_scan_kernel") or "tract_map_kernel" in name:
                others.setdefault(name, []).append(t)
    ours.sort()
    out = dict(trace=path, refine={}, beside={})

    def stats(d):
        return dict(launches=len(d), median_us=round(statistics.median(d), 2), mean_us=round(statistics.fmean(d), 2), min_us=round(min(d), 2), max_us=round(max(d), 2))
    for a, (key, _unit) in enumerate(ARMS):
        d = [x[1] / 1000.0 for i, x in enumerate(ours) if i % len(ARMS) == a and i // len(ARMS) >= 1 + warmup]
        if d:
            out["refine"][key] = stats(d)
    for name, ts in others.items():
        d = [x[1] / 1000.0 for x in sorted(ts)]
        d = d[2 + warmup:] if len(d) > 2 + warmup else d          # (the set-up launches and the warm-up rounds come first)
        out["beside"][name] = stats(d)
    print(json.dumps(out))
    return 0 if out["refine"] else 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", help="a kernel_trace.csv of rocprofv3 --kernel-trace: print the time per launch of every arm")
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--len", type=int, default=15000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.check:
        return check(args.check, args.warmup)
    import numpy as np
    from topsicle_amd import allsteps, hiplib, refine, synth
    sc = hiplib.HipScanner(0)
    unit = "CCCTAA"
    bases, offsets, _ = synth.make_reads(args.reads, args.len, unit, 20261020, errors=synth.ONT)
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
    begin, end = np.full(n, REGION[0], np.int32), np.full(n, REGION[1], np.int32)
    at = refine.regions(res, 100, 6, 20000, 6)[2]

    def scan():
        sc.scan(0, prm)
        sc.sync()
    arms = {key: (lambda u=u: sc.boundary_refine(0, u, tails, begin, end, at)) for key, u in ARMS}
    arms["tract_map"] = lambda: sc.tract_map(0, unit)
    arms["config2_scan"] = scan
    seen = {}
    for name, call in arms.items():                # (the set-up round, one launch per arm in arm order: check() counts on it)
        out = call()
        if name in dict(ARMS):
            stored = at > 0
            seen[name] = dict(score_median=float(np.median(out["score"])), clean_of_the_first_500=int(sum(
                refine.classify(int(r["score"]), int(r["drop"]), None if r["runner_pos"] < 0 else int(r["score"]) - int(r["runner"])) == "clean" for r in out[:500])),
                shift_median_of_stored=float(np.median(np.abs(out["pos"][stored] - at[stored]))) if stored.any() else None)
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
    print(json.dumps(dict(reads=args.reads, read_len=args.len, region=REGION, calls=args.calls, device=sc.device_info(), scan_kernel=sc.kernel_info(0),
                          scan_event_us_per_launch=round(1000.0 * mean_ms, 2), scan_event_launches=n_launches, first_call=seen,
                          host_ms_per_call={name: round(1000.0 * statistics.median(s), 3) for name, s in spent.items()})))
    sc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
