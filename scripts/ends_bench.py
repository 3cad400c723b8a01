#!/usr/bin/env python3
"""Kernel times of the end groups: the sketch (tps_batch_end_sketch) beside the config-2 scan and the variant census on one resident
batch, and the links (tps_sketch_links) beside their numpy restatement.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/ends_bench.py      # the workload
    scripts/ends_bench.py --check DIR/.../<pid>_kernel_trace.csv                                       # time per launch and arm

The workload, alternating in one process and on one context:
  * the config-2 scan of 10 000 x 15 kb synthetic ONT CCCTAA reads (bench.py's `value` region), one launch per call;
  * the variant census of the tracts that scan calls (bin 500, 40 bins), one launch per call;
  * the end sketch of the windows behind those boundaries (k 12, 256 buckets, span 2000), one launch per call;
  * the links of n = 2000 and n = 20 000 sketches of 256 buckets (random, 1 % of them in planted groups of 10; min_match 6,
    max_links 64), one launch per call -- and `match >= min_match` over all pairs in numpy on the host's CPUs, the thing the kernel
    replaces, once per n (blocked so that a block of the compare fits the caches; its time is the host's, not the profiler's).
No bar is set: nobody has measured these kernels before.  The kernels' times come from the profiler's dispatch timestamps (device
clocks); the launches of the two link arms are told apart by their order, which the script fixes.  Without a profiler the script
prints the host's time per call (table / sketches uploaded, launch, kernel, outputs copied back) and, for the scan, the library's
own device-event time per launch."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LINK_N = (2000, 20000)


def _stats(d):
    return dict(launches=len(d), median_us=round(statistics.median(d), 2), mean_us=round(statistics.fmean(d), 2), min_us=round(min(d), 2), max_us=round(max(d), 2))


def check(path, warmup, link_calls):
    """Link dispatches in start order: the first len(LINK_N) are the set-up launches, one per n in order, then link_calls per n."""
    sketch, links, census, scans = [], [], [], {}
    with open(path, newline="") as fh:
        for row in sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"])):
            name = row["Kernel_Name"].split("(")[0].strip()
            d = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0
            if "end_sketch_kernel" in name:
                sketch.append(d)
            elif "sketch_links_kernel" in name:
                links.append(d)
            elif "variant_census_kernel" in name:
                census.append(d)
            elif name.startswith("tps_scan_kernel"):
                scans.setdefault(name, []).append(d)
    out = dict(trace=path, end_sketch={}, sketch_links={}, variant_census={}, scan={})
    if len(sketch) > 1 + warmup:
        out["end_sketch"]["CCCTAA"] = _stats(sketch[1 + warmup:])
    body = links[len(LINK_N):]
    for a, n in enumerate(LINK_N):
        d = body[a * link_calls:(a + 1) * link_calls]
        if d:
            out["sketch_links"][f"n{n}"] = _stats(d)
    if len(census) > 1 + warmup:
        out["variant_census"]["CCCTAA"] = _stats(census[1 + warmup:])
    for name, d in scans.items():
        out["scan"][name] = _stats(d[2 + warmup:] if len(d) > 2 + warmup else d)
    print(json.dumps(out))
    return 0 if out["end_sketch"] else 2


def random_sketches(np, n, buckets=256, seed=5):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 0xFFFFFFF0, (n, buckets), dtype=np.uint32)
    groups = max(1, n // 1000)
    centre = rng.integers(0, 0xFFFFFFF0, (groups, buckets), dtype=np.uint32)
    for i in range(10 * groups):
        cols = rng.choice(buckets, 40, replace=False)
        s[i, cols] = centre[i % groups, cols]
    s[rng.random((n, buckets)) < 0.05] = 0xFFFFFFFF
    return s


def numpy_links(np, s, min_match, threads):
    """degree[i] = the j > i with match(i, j) >= min_match, in numpy: blocks of rows against all rows behind them, on `threads`
    threads (numpy's compare and sum release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    n = len(s)
    filled = s != 0xFFFFFFFF
    degree = np.zeros(n, np.int64)

    def rows(lo):
        hi = min(n, lo + 8)
        for i in range(lo, hi):
            m = ((s[i + 1:] == s[i]) & filled[i]).sum(axis=1)
            degree[i] = int((m >= min_match).sum())
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(rows, range(0, n, 8)))
    return degree


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", help="a kernel_trace.csv of rocprofv3 --kernel-trace: print the time per launch of every arm")
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--len", type=int, default=15000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--link-calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--numpy-threads", type=int, default=16)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    if args.check:
        return check(args.check, args.warmup, args.link_calls)
    import numpy as np
    from topsicle_amd import allsteps, ends, hiplib, synth, variants
    sc = hiplib.HipScanner(0)
    unit, no_bp = "CCCTAA", 1000
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
    begin, end = variants.tract_bounds(res, 100, len(unit), 20000)
    tails = np.where(end > begin, res["tail"], 0).astype(np.uint8)
    e_begin, e_end = ends.windows(res, 100, len(unit), 20000, ends.DEFAULT_SPAN)
    sc.variant_census(0, unit, tails, begin, end)
    sk, kept = sc.end_sketch(0, unit, tails, e_begin, e_end)
    sets = {n: random_sketches(np, n) for n in LINK_N}
    link_found = {}
    for n, s in sets.items():                      # (the set-up launches of the links, one per n in order: check() counts on it)
        degree, links, _ = sc.sketch_links(s, ends.DEFAULT_MIN_MATCH, ends.DEFAULT_MAX_LINKS)
        link_found[f"n{n}"] = dict(edges=int(degree.sum()), rows_with_links=int((degree > 0).sum()))
        link_found[f"n{n}"]["degree"] = degree

    def scan():
        sc.scan(0, prm)
        sc.sync()
    arms = {"end_sketch": lambda: sc.end_sketch(0, unit, tails, e_begin, e_end),
            "variant_census": lambda: sc.variant_census(0, unit, tails, begin, end),
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
    for n, s in sets.items():
        d = []
        for _ in range(args.link_calls):
            t0 = time.perf_counter()
            sc.sketch_links(s, ends.DEFAULT_MIN_MATCH, ends.DEFAULT_MAX_LINKS)
            d.append(time.perf_counter() - t0)
        host_ms[f"sketch_links_n{n}"] = round(1000.0 * statistics.median(d), 3)
    numpy_ms = {}
    for n, s in sets.items():
        want = link_found[f"n{n}"].pop("degree")
        if args.no_numpy:
            continue
        t0 = time.perf_counter()
        got = numpy_links(np, s, ends.DEFAULT_MIN_MATCH, args.numpy_threads)
        numpy_ms[f"n{n}"] = round(1000.0 * (time.perf_counter() - t0), 1)
        assert np.array_equal(got, want), "numpy and the kernel disagree on the degrees"
    report = dict(reads=args.reads, read_len=args.len, calls=args.calls, device=sc.device_info(), scan_kernel=sc.kernel_info(0),
                  scan_event_us_per_launch=round(1000.0 * mean_ms, 2), scan_event_launches=n_launches, host_ms_per_call=host_ms,
                  numpy_threads=args.numpy_threads, numpy_ms=numpy_ms, links=link_found,
                  sketch=dict(windows=int((e_end > e_begin).sum()), kept_per_window=round(float(kept[e_end > e_begin].mean()), 1),
                              filled_buckets_per_window=round(float((sk[e_end > e_begin] != 0xFFFFFFFF).sum(axis=1).mean()), 1)))
    print(json.dumps(report))
    sc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
