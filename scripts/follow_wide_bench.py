#!/usr/bin/env python3
"""Kernel time of the wide followers kernel (tps_followers_kernel_wide) beside the narrow one it is measured against.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/follow_wide_bench.py      # the workload
    scripts/follow_wide_bench.py --case a --check DIR/.../<pid>_kernel_stats.csv                             # the verdict

The workload, on 4000 x 15 kb synthetic reads (bases 100..2000 of both strands, reads longer than 9000), the calls of one
comparison alternating in ONE process, two contexts per table so that no call waits for a table switch:
  (a) a 15-letter motif at k = 13 (15 k-mers, 2 following letters, with the histogram): tps_batch_kmer_followers on the narrow
      table and tps_batch_kmer_followers_wide on the same table set with tps_set_patterns_wide;
  (b) the 23-letter motif at the reference's default k = 21 through the wide kernel (on reads of its own motif), in a process of its own
      (--case b), so that (a)'s average of tps_followers_kernel_wide holds (a)'s launches only.
Every call is one launch.  --check reads rocprofv3's kernel statistics and prints the two kernels' averages; for case (a) the
guard is wide <= 2 x narrow (exit status 1 when missed, 2 when a kernel the case launches is not in the file): the wide kernel builds 64- instead of 32-bit codes -- four staged
dwords and extra funnel shifts per position -- and compares bytes where the narrow one reads ready-made pattern masks.
Without a profiler the script prints the host's time per call (launch, kernel, picks copied back)."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M15, M23 = "ACGGATGTCTAACTT", "ACGGATGTCTAACTTCTTGGTGT"
NARROW, WIDE = "tps_followers_kernel", "tps_followers_kernel_wide"


def check(path, case):
    avg = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Name"].split("(")[0].strip()
            if name in (NARROW, WIDE):
                avg[name] = dict(calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) / 1000.0, 2),
                                 min_us=round(float(row["MinNs"]) / 1000.0, 2), max_us=round(float(row["MaxNs"]) / 1000.0, 2))
    out = dict(stats=path, case=case, kernels=avg)
    need = (NARROW, WIDE) if case == "a" else (WIDE,)
    missing = [name for name in need if name not in avg]
    if missing:
        out["error"] = "no launches of " + ", ".join(missing) + " in the statistics"
        print(json.dumps(out))
        return 2
    ok = True
    if case == "a":
        out["wide_over_narrow"] = round(avg[WIDE]["average_us"] / avg[NARROW]["average_us"], 3)
        ok = out["wide_over_narrow"] <= 2.0
        out["guard_met"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", help="a kernel_stats.csv of rocprofv3 --kernel-trace --stats: print the averages, judge the guard")
    ap.add_argument("--case", choices=["a", "b"], default="a")
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--len", type=int, default=15000)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.check:
        return check(args.check, args.case)
    from topsicle_amd import allsteps, hiplib, synth
    motif, k = (M15, 13) if args.case == "a" else (M23, 21)
    table = allsteps.patterns_to_search(motif, k)
    n_fwd, follow = len(table) // 2, len(motif) - k
    bases, offsets, _ = synth.make_reads(args.reads, args.len, motif, 20261017, errors=synth.ONT)
    arms = {}
    wide = hiplib.HipScanner(0)
    wide.set_patterns_wide(table)
    wide.upload(0, bases, offsets)
    arms[WIDE] = lambda: wide.kmer_followers_wide(0, n_fwd, follow, 100, 2000, 9000)
    narrow = None
    if args.case == "a":
        narrow = hiplib.HipScanner(0)
        narrow.set_patterns(table)
        narrow.upload(0, bases, offsets)
        arms[NARROW] = lambda: narrow.kmer_followers(0, n_fwd, follow, 100, 2000, 9000)
    spent = {name: 0.0 for name in arms}
    picks = {}
    for i in range(args.warmup + args.calls):
        for name, call in arms.items():
            t0 = time.perf_counter()
            p, h = call()
            if i >= args.warmup:
                spent[name] += time.perf_counter() - t0
            picks[name] = (p, h)
    if narrow is not None:
        import numpy as np
        assert np.array_equal(picks[WIDE][0], picks[NARROW][0]) and np.array_equal(picks[WIDE][1], picks[NARROW][1]), "the two kernels disagree"
    print(json.dumps(dict(case=args.case, motif=motif, k=k, n_fwd=n_fwd, follow=follow, reads=args.reads, read_len=args.len, calls=args.calls,
                          device=wide.device_info(), picks=int(picks[WIDE][1].sum()),
                          host_ms_per_call={name: round(1000.0 * s / args.calls, 3) for name, s in spent.items()})))
    wide.close()
    if narrow is not None:
        narrow.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
