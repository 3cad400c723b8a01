#!/usr/bin/env python3
"""Kernel time of the adapter search (tps_batch_adapter_find) beside the config-2 scan and the variant census, on one resident batch.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/adapter_bench.py      # the workload
    scripts/adapter_bench.py --check DIR/.../<pid>_kernel_trace.csv                                       # time per launch and arm

The workload: 10 000 x 15 kb synthetic ONT reads (the benchmark's config 2 shape, CCCTAA), resident in one slot and scanned once with
the config-2 parameters; every read is searched in its first 256 bases (every read, not only those with a stored boundary: the
kernel's time does not depend on what the region holds).  Then, alternating in one process and on one context:
  * the adapter search with P = 1, 12 and 64 random patterns of m = 24 and of m = 64 letters, one launch per call (six arms);
  * the variant census of the same batch against CCCTAA (bin 500, 40 bins, with the profile);
  * the config-2 scan (bench.py's `value` region: step 1, windows, change point, sums stored).
No bar is set: nobody has measured this kernel before.  The kernels' times come from the profiler's dispatch timestamps (device
clocks); the launches of the adapter arms are told apart by their order, which the script fixes.  Without a profiler the script prints
the host's time per call."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNEL = "adapter_find_kernel"
ARMS = [(P, m) for m in (24, 64) for P in (1, 12, 64)]
SEARCH = 256


def check(path, warmup):
    """Adapter dispatches in start order: launch i belongs to arm i mod 6 (after the set-up round main() makes, one launch per arm in
    the same order); the first `warmup` rounds are left out."""
    ours, others = [], {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"].split("(")[0].strip()
            t = (int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
            if KERNEL in name:
                ours.append(t)
            elif name.startswith("tps_scan_kernel") or "variant_census_kernel" in name:
                others.setdefault(name, []).append(t)
    ours.sort()
    out = dict(trace=path, adapter={}, beside={})
    for a, (P, m) in enumerate(ARMS):
        d = [x[1] / 1000.0 for i, x in enumerate(ours) if i % len(ARMS) == a and i // len(ARMS) >= 1 + warmup]
        if d:
            out["adapter"][f"P{P}_m{m}"] = dict(launches=len(d), median_us=round(statistics.median(d), 2), mean_us=round(statistics.fmean(d), 2),
                                                min_us=round(min(d), 2), max_us=round(max(d), 2))
    for name, ts in others.items():
        d = [x[1] / 1000.0 for x in sorted(ts)]
        d = d[2 + warmup:] if len(d) > 2 + warmup else d          # (the set-up launches and the warm-up rounds come first)
        out["beside"][name] = dict(launches=len(d), median_us=round(statistics.median(d), 2), mean_us=round(statistics.fmean(d), 2), min_us=round(min(d), 2), max_us=round(max(d), 2))
    print(json.dumps(out))
    return 0 if out["adapter"] else 2


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
    from topsicle_amd import allsteps, hiplib, synth, variants
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
    begin, end = variants.tract_bounds(res, 100, 6, 20000)
    tails = np.where(end > begin, res["tail"], 0).astype(np.uint8)
    n = args.reads
    a_tails, a_begin, a_end = res["tail"].astype(np.uint8), np.zeros(n, np.int32), np.full(n, SEARCH, np.int32)
    rng = np.random.default_rng(19)
    sets = {(P, m): ["".join("ACGT"[j] for j in rng.integers(0, 4, m)) for _ in range(P)] for P, m in ARMS}

    def scan():
        sc.scan(0, prm)
        sc.sync()
    arms = {f"P{P}_m{m}": (lambda k=(P, m): sc.adapter_find(0, sets[k], a_tails, a_begin, a_end)) for P, m in ARMS}
    arms["variant_census"] = lambda: sc.variant_census(0, unit, tails, begin, end)
    arms["config2_scan"] = scan
    best = {}
    for name, call in arms.items():                # (the set-up round, one launch per arm in arm order: check() counts on it)
        out = call()
        if name.startswith("P"):
            best[name] = int(out[0].min())
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
    print(json.dumps(dict(reads=args.reads, read_len=args.len, search=SEARCH, calls=args.calls, device=sc.device_info(), scan_kernel=sc.kernel_info(0),
                          scan_event_us_per_launch=round(1000.0 * mean_ms, 2), scan_event_launches=n_launches, reads_with_tract=int((end > begin).sum()),
                          smallest_distance_of_random_patterns=best,
                          host_ms_per_call={name: round(1000.0 * statistics.median(s), 3) for name, s in spent.items()})))
    sc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
