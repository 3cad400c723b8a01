#!/usr/bin/env python3
"""Kernel times of the anchoring: the window extraction (tps_batch_end_window) beside the end sketch and the config-2 scan on one
resident batch, and the offsets (tps_window_offsets) of 20 000 windows in groups of 12.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/anchor_bench.py     # the workload
    scripts/anchor_bench.py --check DIR/.../<pid>_kernel_trace.csv                                      # time per launch and arm

The workload, alternating in one process and on one context:
  * the config-2 scan of 10 000 x 15 kb synthetic ONT CCCTAA reads (bench.py's `value` region), one launch per call;
  * the end sketch of the windows behind the boundaries that scan calls (k 12, 256 buckets, span 2000), one launch per call;
  * the window extraction of the same windows (k 12, span 2000), one launch per call;
  * the offsets of 20 000 rows of 2000 bases (k 12): 1667 groups of 12 windows cut from one random subtelomere each at a jitter of
    0 .. 600 bases with 4 % substitutions, every position kept (the most a window can hold; extracted windows keep about two
    thirds), every row against the first row of its group; one launch per call.
No bar is set: nobody has measured these kernels before.  The kernels' times come from the profiler's dispatch timestamps (device
clocks).  Without a profiler the script prints the host's time per call (inputs uploaded, launch, kernel, outputs copied back) and,
for the scan, the library's own device-event time per launch -- the library records events around scan launches only."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = {"end_window_kernel": "end_window", "window_offsets_kernel": "window_offsets", "end_sketch_kernel": "end_sketch"}


def _stats(d):
    return dict(launches=len(d), median_us=round(statistics.median(d), 2), mean_us=round(statistics.fmean(d), 2), min_us=round(min(d), 2), max_us=round(max(d), 2))


def check(path, warmup):
    """Dispatches in start order; the first 1 + warmup of every arm (set-up, warm-up) are left out."""
    arms, scans = {}, {}
    with open(path, newline="") as fh:
        for row in sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"])):
            name = row["Kernel_Name"].split("(")[0].strip()
            d = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0
            for key, arm in ARMS.items():
                if key in name:
                    arms.setdefault(arm, []).append(d)
            if name.startswith("tps_scan_kernel"):
                scans.setdefault(name, []).append(d)
    out = dict(trace=path, scan={})
    for arm, d in arms.items():
        if len(d) > 1 + warmup:
            out[arm] = _stats(d[1 + warmup:])
    for name, d in scans.items():
        out["scan"][name] = _stats(d[2 + warmup:] if len(d) > 2 + warmup else d)
    print(json.dumps(out))
    return 0 if "window_offsets" in out and "end_window" in out else 2


def grouped_windows(np, n, span, per_group=12, jitter=600, sub_rate=0.04, seed=7):
    """(codes, keep, length, ref, planted offset against the reference): n windows of `span` letters in groups of per_group."""
    rng = np.random.default_rng(seed)
    groups = (n + per_group - 1) // per_group
    subs = rng.integers(0, 4, (groups, span + jitter), dtype=np.uint8)
    start = rng.integers(0, jitter + 1, n)
    g = np.arange(n) // per_group
    letters = subs[g[:, None], start[:, None] + np.arange(span)[None, :]]
    hit = rng.random((n, span)) < sub_rate
    letters = np.where(hit, rng.integers(0, 4, (n, span), dtype=np.uint8), letters).astype(np.uint32)
    cdw, kdw = (span + 15) // 16, (span + 31) // 32
    pad = np.zeros((n, cdw * 16), np.uint32)
    pad[:, :span] = letters
    codes = (pad.reshape(n, cdw, 16) << (2 * np.arange(16, dtype=np.uint32))[None, None, :]).sum(axis=2, dtype=np.uint64).astype(np.uint32)
    bits = np.zeros((n, kdw * 32), np.uint32)
    bits[:, :span - 11] = 1
    keep = (bits.reshape(n, kdw, 32) << np.arange(32, dtype=np.uint32)[None, None, :]).sum(axis=2, dtype=np.uint64).astype(np.uint32)
    ref = (g * per_group).astype(np.int32)
    return codes, keep, np.full(n, span, np.int32), ref, (start - start[ref]).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", help="a kernel_trace.csv of rocprofv3 --kernel-trace: print the time per launch of every arm")
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--len", type=int, default=15000)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--offset-calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.check:
        return check(args.check, args.warmup)
    import numpy as np
    from topsicle_amd import allsteps, ends, hiplib, synth
    sc = hiplib.HipScanner(0)
    unit, no_bp, span, k = "CCCTAA", 1000, ends.DEFAULT_SPAN, ends.DEFAULT_K
    bases, offsets, _ = synth.make_reads(args.reads, args.len, unit, 20261019, errors=synth.ONT)
    sc.upload(0, bases, offsets)
    pats = allsteps.patterns_to_search(telopattern=unit, cut_length=4)
    prm = hiplib.make_params(no_bp=no_bp, min_len=9000, min_count=allsteps.min_count_for_cutoff(0.7, no_bp / len(unit), no_bp), window=100, slide=len(unit),
                             trimfirst=100, maxlen=20000, jump=5, min_size=2, flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS)
    hiplib.set_table(sc, pats)
    for _ in range(2):
        sc.scan(0, prm)
        sc.sync()
    res = sc.results(0)
    hiplib.resolve_ties(sc, 0, res, len(pats), prm.jump, prm.min_size)
    e_begin, e_end = ends.windows(res, 100, len(unit), 20000, span)
    tails = np.where(e_end > e_begin, res["tail"], 0).astype(np.uint8)
    sk, kept = sc.end_sketch(0, unit, tails, e_begin, e_end)
    codes, keep = sc.end_window(0, unit, tails, e_begin, e_end, k, span)
    n_keep = np.array([bin(int.from_bytes(row.tobytes(), "little")).count("1") for row in keep])
    assert np.array_equal(n_keep, kept), "popcount(keep) differs from the sketch's kept"
    g_codes, g_keep, g_len, g_ref, planted = grouped_windows(np, args.rows, span)
    offset, votes, second = sc.anchor_offsets(g_codes, g_keep, g_len, g_ref, span, k)         # (the set-up launch)
    right = int((offset == planted).sum())

    def scan():
        sc.scan(0, prm)
        sc.sync()
    arms = {"end_window": lambda: sc.end_window(0, unit, tails, e_begin, e_end, k, span),
            "end_sketch": lambda: sc.end_sketch(0, unit, tails, e_begin, e_end),
            "config2_scan": scan}
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
    host_ms = {name: round(1000.0 * statistics.median(s), 3) for name, s in spent.items()}
    d = []
    for i in range(args.warmup + args.offset_calls):
        t0 = time.perf_counter()
        sc.anchor_offsets(g_codes, g_keep, g_len, g_ref, span, k)
        if i >= args.warmup:
            d.append(time.perf_counter() - t0)
    host_ms["window_offsets"] = round(1000.0 * statistics.median(d), 3)
    report = dict(reads=args.reads, read_len=args.len, rows=args.rows, calls=args.calls, device=sc.device_info(), scan_kernel=sc.kernel_info(0),
                  scan_event_us_per_launch=round(1000.0 * mean_ms, 2), scan_event_launches=n_launches, host_ms_per_call=host_ms,
                  windows=dict(windows=int((e_end > e_begin).sum()), kept_per_window=round(float(kept[e_end > e_begin].mean()), 1)),
                  offsets=dict(rows=args.rows, offsets_equal_to_planted=right, votes_median=float(np.median(votes)), second_max=int(second.max())))
    print(json.dumps(report))
    sc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
