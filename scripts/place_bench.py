#!/usr/bin/env python3
"""Kernel and call times of the placement (tps_window_place) beside the only thing that could do its work before it existed:
tps_window_offsets called once per reference row over all the queries.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/place_bench.py     # the workload
    scripts/place_bench.py --check DIR/.../<pid>_kernel_trace.csv                                     # time per launch and arm
    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_WAVE_CYCLES --output-format csv -d DIR -- python3 scripts/place_bench.py --no-baseline
    scripts/place_bench.py --counters DIR/.../<pid>_counter_collection.csv                            # counters per launch and arm

The workload, alternating in one process and on one context, `--rounds` times after `--warmup` rounds:
  * place92:    20 000 query rows of 2 000 bases (k 12) against R = 92 reference rows, one call = one launch;
  * place1024:  the same number of rows against R = 1 024 reference rows;
  * baseline92: tps_window_offsets over the rows of place92, once per reference row: 92 calls = 92 launches.
The rows are cut as scripts/anchor_bench.py cuts them: groups of 20 000 // R windows, every group's from one random subtelomere at a
jitter of 0 .. 600 bases with 4 % substitutions, every position kept; the reference rows are the first window of the first R groups
(the few rows left over belong to no reference end).  Every arm's
answers are checked against the planted group and offset before anything is timed.  No ratio is set in advance: place92 must be
below baseline92.  The kernels' times come from the profiler's dispatch timestamps (device clocks); without a profiler the script
prints the host's time per call (index built, inputs uploaded, launch, kernel, outputs copied back)."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

REFS = (92, 1024)


def _stats(d):
    return dict(launches=len(d), median_us=round(statistics.median(d), 2), mean_us=round(statistics.fmean(d), 2), min_us=round(min(d), 2), max_us=round(max(d), 2))


def _dispatches(path, column):
    """{kernel: [(start or dispatch id, value)]} of a rocprofv3 csv, in dispatch order"""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"].split("(")[0].strip()
            for key in ("window_place_kernel", "window_offsets_kernel"):
                if key in name:
                    out.setdefault(key, []).append((int(row.get("Start_Timestamp") or row["Dispatch_Id"]), row if column is None else float(row[column])))
    return {k: [v for _, v in sorted(d, key=lambda t: t[0])] for k, d in out.items()}


def check(path, warmup, baseline):
    """place launches alternate R = 92, R = 1 024 (the two set-up launches first); the baseline's come 92 to a round."""
    rows = _dispatches(path, None)
    place = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0 for r in rows.get("window_place_kernel", [])]
    out = dict(trace=path)
    skip = 2 * (1 + warmup)
    for j, R in enumerate(REFS):
        d = place[skip + j::2]
        if d:
            out[f"place{R}"] = _stats(d)
    offs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0 for r in rows.get("window_offsets_kernel", [])]
    if baseline and offs:
        per_round = [sum(offs[i:i + REFS[0]]) for i in range(REFS[0] * (1 + warmup), len(offs) - REFS[0] + 1, REFS[0])]
        out["baseline92_sum_of_92_launches"] = _stats(per_round)
        out["baseline92_one_launch"] = _stats(offs[REFS[0] * (1 + warmup):])
    print(json.dumps(out))
    return 0 if "place92" in out else 2


def counters(path, warmup):
    """mean per launch of every counter, per arm"""
    per = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            if "window_place_kernel" in row["Kernel_Name"]:
                per.setdefault(row["Counter_Name"], []).append((int(row["Dispatch_Id"]), float(row["Counter_Value"])))
    out = dict(counters=path)
    for name, d in per.items():
        v = [x for _, x in sorted(d)]
        for j, R in enumerate(REFS):
            mine = v[2 * (1 + warmup) + j::2]
            if mine:
                out.setdefault(f"place{R}", {})[name] = round(statistics.fmean(mine), 1)
    print(json.dumps(out))
    return 0 if "place92" in out else 2


def workload(np, n, R, span):
    from anchor_bench import grouped_windows
    per_group = n // R                             # (the rows left over form groups of their own: reads of ends the reference lacks)
    codes, keep, length, ref, planted = grouped_windows(np, n, span, per_group=per_group, seed=7 + R)
    first = np.arange(R, dtype=np.int64) * per_group
    group = (ref // per_group).astype(np.int32)
    return dict(codes=codes, keep=keep, length=length, group=group, known=group < R, first=first, planted=planted, R=R)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", help="a kernel_trace.csv of rocprofv3 --kernel-trace: print the time per launch of every arm")
    ap.add_argument("--counters", help="a counter_collection.csv of rocprofv3 --pmc: print the counters per launch of the place arms")
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true", help="leave the 92-call baseline out (counter runs)")
    args = ap.parse_args()
    if args.check:
        return check(args.check, args.warmup, not args.no_baseline)
    if args.counters:
        return counters(args.counters, args.warmup)
    import numpy as np
    from topsicle_amd import ends, hiplib
    sc = hiplib.HipScanner(0)
    span, k = ends.DEFAULT_SPAN, ends.DEFAULT_K
    sets = {R: workload(np, args.rows, R, span) for R in REFS}

    def place(R):
        w = sets[R]
        return sc.place_windows(w["codes"], w["keep"], w["length"], w["codes"][w["first"]], w["keep"][w["first"]], w["length"][w["first"]], span, k)

    def baseline():
        w = sets[REFS[0]]
        return [sc.anchor_offsets(w["codes"], w["keep"], w["length"], np.full(args.rows, r, np.int32), span, k) for r in w["first"]]
    report = dict(rows=args.rows, span=span, k=k, rounds=args.rounds, device=sc.device_info(), answers={})
    for R in REFS:                                 # (the set-up launches: the answers)
        w = sets[R]
        ref, total, runner_ref, runner, offset, votes, second = place(R)
        kn = w["known"]
        report["answers"][f"place{R}"] = dict(rows_of_known_ends=int(kn.sum()), on_their_end=int((ref[kn] == w["group"][kn]).sum()),
                                              offsets_equal_to_planted=int((offset[kn] == w["planted"][kn]).sum()), votes_median=float(np.median(votes[kn])),
                                              second_max=int(second.max()), runner_max=int(runner.max()), votes_max_of_the_other_rows=int(votes[~kn].max()))
    if not args.no_baseline:
        w = sets[REFS[0]]
        offs = baseline()
        votes = np.stack([o[1] for o in offs])
        best = votes.argmax(axis=0)
        kn = w["known"]
        report["answers"]["baseline92"] = dict(on_their_end=int((best[kn] == w["group"][kn]).sum()),
                                               offsets_equal_to_planted=int((np.stack([o[0] for o in offs])[best, np.arange(args.rows)][kn] == w["planted"][kn]).sum()))
    arms = {f"place{R}": (lambda R=R: place(R)) for R in REFS}
    if not args.no_baseline:
        arms["baseline92"] = baseline
    spent = {name: [] for name in arms}
    for i in range(args.warmup + args.rounds):
        for name, call in arms.items():
            t0 = time.perf_counter()
            call()
            if i >= args.warmup:
                spent[name].append(time.perf_counter() - t0)
    report["host_ms_per_arm"] = {name: dict(median=round(1000.0 * statistics.median(s), 3), min=round(1000.0 * min(s), 3)) for name, s in spent.items()}
    print(json.dumps(report))
    sc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
