#!/usr/bin/env python3
"""Kernel and whole-call times of the banded alignment (tps_window_align) beside the offsets (tps_window_offsets) on the same rows.

    scripts/consensus_bench.py --out profiles/r24_consensus                                                # host time per call -> host_times.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/consensus_bench.py     # the workload under the profiler
    scripts/consensus_bench.py --check DIR/.../<pid>_kernel_trace.csv --out profiles/r24_consensus         # time per launch and arm -> kernel_times.json

The workload: 20 000 rows of 2 000 letters in 1 667 groups of 12 -- every group one random subtelomere, every row a copy cut at a
jitter of 0 .. 300 bases and mutated at synth.ONT's substitution / insertion / deletion rates, every position kept -- each row against
the first row of its group.  One context, alternating:
  * the offsets of the rows (k 12), one launch per call;
  * the alignment of the rows on those offsets, one pile row per group and no cols (the first pass of topsicle_amd/consensus.py), one
    launch and the pile's clearing per call;
  * the same alignment with every centre at 4096: the band lies beside the matrix, so the kernel walks the same band rows (the
    forward pass executes the same instructions whatever the letters are) and ends before the traceback and the pile.  Full minus
    forward-only is what the traceback and the outputs cost.
No bar is set: nothing earlier does this work.  The kernels' times come from the profiler's dispatch timestamps (device clocks);
without a profiler the script prints the host's time per call (inputs uploaded, launch, kernel, outputs copied back)."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = {"window_align_kernel": "window_align", "window_offsets_kernel": "window_offsets"}


def _stats(d):
    return dict(launches=len(d), median_us=round(statistics.median(d), 2), mean_us=round(statistics.fmean(d), 2), min_us=round(min(d), 2), max_us=round(max(d), 2))


def _emit(report, out):
    print(json.dumps(report))
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "kernel_times.json" if "trace" in report else "host_times.json"), "w") as fh:
            fh.write(json.dumps(report, indent=1) + "\n")


def check(path, warmup, out_dir):
    """Dispatches in start order; the first 1 + warmup of every arm (set-up, warm-up) are left out.  The alignment's launches behind
    the set-up one alternate: full, forward only."""
    arms = {}
    with open(path, newline="") as fh:
        for row in sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"])):
            name = row["Kernel_Name"].split("(")[0].strip()
            for key, arm in ARMS.items():
                if key in name:
                    arms.setdefault(arm, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
    out = dict(trace=os.path.basename(path))
    both = arms.pop("window_align", [])[1:]
    arms["window_align"], arms["window_align_forward_only"] = both[0::2], both[1::2]
    for arm, d in arms.items():
        if len(d) > (1 if arm == "window_offsets" else 0) + warmup:
            out[arm] = _stats(d[(1 if arm == "window_offsets" else 0) + warmup:])
    _emit(out, out_dir)
    return 0 if "window_align" in out and "window_align_forward_only" in out and "window_offsets" in out else 2


def grouped_rows(np, synth, n, span, per_group=12, jitter=300, seed=24):
    """(codes, keep, length, ref): n windows of up to `span` letters in groups of per_group, mutated at synth.ONT's rates."""
    rng = np.random.default_rng(seed)
    sub, ins, dele = synth.ONT
    groups = (n + per_group - 1) // per_group
    subs = rng.integers(0, 4, (groups, span + jitter + span // 8), dtype=np.uint8)
    cdw, kdw = (span + 15) // 16, (span + 31) // 32
    letters = np.zeros((n, cdw * 16), np.uint32)
    length = np.zeros(n, np.int32)
    for i in range(n):
        src = subs[i // per_group, int(rng.integers(0, jitter + 1)):]
        r = rng.random((len(src), 3))
        src = np.where(r[:, 0] < sub, rng.integers(0, 4, len(src), dtype=np.uint8), src)[r[:, 2] >= dele]
        extra = np.nonzero(r[r[:, 2] >= dele, 1] < ins)[0]
        src = np.insert(src, extra, rng.integers(0, 4, len(extra), dtype=np.uint8))[:span]
        letters[i, :len(src)] = src
        length[i] = len(src)
    codes = (letters.reshape(n, cdw, 16) << (2 * np.arange(16, dtype=np.uint32))[None, None, :]).sum(axis=2, dtype=np.uint64).astype(np.uint32)
    bits = (np.arange(kdw * 32)[None, :] < (length - 11)[:, None]).astype(np.uint32)
    keep = (bits.reshape(n, kdw, 32) << np.arange(32, dtype=np.uint32)[None, None, :]).sum(axis=2, dtype=np.uint64).astype(np.uint32)
    return codes, keep, length, ((np.arange(n) // per_group) * per_group).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", help="a kernel_trace.csv of rocprofv3 --kernel-trace: print the time per launch of every arm")
    ap.add_argument("--out", help="a directory: the report is also written there (host_times.json, with --check kernel_times.json)")
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--span", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.check:
        return check(args.check, args.warmup, args.out)
    import numpy as np
    from topsicle_amd import hiplib, synth
    codes, keep, length, ref = grouped_rows(np, synth, args.rows, args.span)
    group = (ref // 12).astype(np.int32)
    n_groups = int(group.max()) + 1
    ref_rows = np.arange(n_groups) * 12
    sc = hiplib.HipScanner(0)
    offset, votes, second = sc.anchor_offsets(codes, keep, length, ref, args.span, 12)                 # (the set-up launches)
    stat, _cols, pile = sc.align_windows(codes, length, codes[ref_rows], length[ref_rows], group, offset, args.span, cols=False, pile_row=group, n_pile=n_groups)
    far = np.full(args.rows, 4096, np.int32)
    arms = {"window_offsets": lambda: sc.anchor_offsets(codes, keep, length, ref, args.span, 12),
            "window_align": lambda: sc.align_windows(codes, length, codes[ref_rows], length[ref_rows], group, offset, args.span, cols=False, pile_row=group,
                                                     n_pile=n_groups),
            "window_align_forward_only": lambda: sc.align_windows(codes, length, codes[ref_rows], length[ref_rows], group, far, args.span, cols=False,
                                                                  pile_row=group, n_pile=n_groups)}
    spent = {name: [] for name in arms}
    for i in range(args.warmup + args.calls):
        for name, call in arms.items():
            t0 = time.perf_counter()
            call()
            if i >= args.warmup:
                spent[name].append(time.perf_counter() - t0)
    columns = np.maximum(stat[:, 4] - stat[:, 3], 1)
    report = dict(rows=args.rows, span=args.span, groups=n_groups, calls=args.calls, device=sc.device_info(),
                  host_ms_per_call={name: round(1000.0 * statistics.median(s), 3) for name, s in spent.items()},
                  align=dict(none=int((stat[:, 5] & 1 != 0).sum()), edge=int((stat[:, 5] & 2 != 0).sum()), votes_median=float(np.median(votes)),
                             edits_per_1000_columns_median=round(float(np.median(1000.0 * stat[:, 0] / columns)), 1),
                             columns_median=int(np.median(columns)), pile_depth_median=int(np.median(pile[:, 300:1500, :5].sum(axis=2)))))
    _emit(report, args.out)
    sc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
