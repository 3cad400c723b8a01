#!/usr/bin/env python3
"""Kernel time of the motif census (tps_batch_motif_census) beside the step-1-only scan of the same resident batch.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/motif_census_bench.py      # the workload
    scripts/motif_census_bench.py --check DIR/.../<pid>_kernel_stats.csv                                       # the two averages

The workload: 10 000 x 15 kb synthetic ONT reads (CCCTAA, the benchmark's config 2 shape), in one process and on one context
  * the census with its defaults (periods 4..32, bases 0..1000 of both ends, every read), one launch per call;
  * tps_batch_scan with TPS_F_STEP1 alone on the k = 4 table of CCCTAA (the first / last 1000 bases counted against 12 patterns, the
    end picked): the existing kernel that looks at the same bases, one launch per call
alternating.  No bar is set: there is no earlier census to compare with.  Without a profiler the script prints the host's time per
call (launch, kernel, results copied back)."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CENSUS = "motif_census_kernel"


def check(path):
    out = dict(stats=path, kernels={})
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Name"].split("(")[0].strip()
            if CENSUS in name or name.startswith("tps_scan_kernel"):
                out["kernels"][name] = dict(calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) / 1000.0, 2),
                                            min_us=round(float(row["MinNs"]) / 1000.0, 2), max_us=round(float(row["MaxNs"]) / 1000.0, 2))
    print(json.dumps(out))
    return 0 if any(CENSUS in k for k in out["kernels"]) else 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", help="a kernel_stats.csv of rocprofv3 --kernel-trace --stats: print the averages of the two kernels")
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--len", type=int, default=15000)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.check:
        return check(args.check)
    from topsicle_amd import allsteps, hiplib, motif, synth
    bases, offsets, _ = synth.make_reads(args.reads, args.len, "CCCTAA", 20261018, errors=synth.ONT)
    sc = hiplib.HipScanner(0)
    sc.upload(0, bases, offsets)
    hits, _ = sc.motif_census(0)                         # (before any table is set)
    sc.set_patterns(allsteps.patterns_to_search("CCCTAA", 4))
    prm = hiplib.make_params(no_bp=1000, min_len=0, min_count=0, flags=hiplib.F_STEP1)

    def step1():
        sc.scan(0, prm)
        sc.sync()
    arms = {"census": lambda: sc.motif_census(0), "step1_scan": step1}
    spent = {name: 0.0 for name in arms}
    for i in range(args.warmup + args.calls):
        for name, call in arms.items():
            t0 = time.perf_counter()
            call()
            if i >= args.warmup:
                spent[name] += time.perf_counter() - t0
    rows = motif.tally(hits)
    print(json.dumps(dict(reads=args.reads, read_len=args.len, calls=args.calls, device=sc.device_info(), step1_kernel=sc.kernel_info(0),
                          rank1=rows[0][:3] if rows else None, voting_ends=sum(r[2] for r in rows),
                          host_ms_per_call={name: round(1000.0 * s / args.calls, 3) for name, s in spent.items()})))
    sc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
