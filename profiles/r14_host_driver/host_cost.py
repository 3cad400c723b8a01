#!/usr/bin/env python3
"""Host time per scan launch of the library TOPSICLE_HIP_LIB names (default: the tree's own), one JSON line.

The batches are so small that the kernel is shorter than the host's work per launch: the loop is bound by the host, so the wall time
of LAUNCHES scans and one sync, divided by LAUNCHES, is the cost of tps_batch_scan on the planned path (binding included, which is
the same for every library).  `no_events` = 1 (the launch path without the event pool) and = 0, for the fused kernel with the shapes
of config4_1pct's parameters (full pipeline, slide 6, k = 4), step 1 only, and the wide kernel.  ROUNDS rounds per case; the line
holds every round in us per launch."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from topsicle_amd import allsteps, hiplib, synth       # noqa: E402

LAUNCHES, ROUNDS = 4000, 7
FULL = hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS


def main():
    motif = "CCCTAA"
    bases, offsets, _ = synth.make_reads(8, 1200, motif, seed=8, tract_min=300, tract_max=900)
    mc = allsteps.min_count_for_cutoff(0.5, 1000 / len(motif), 1000)
    cases = {"fused_full": (allsteps.patterns_to_search(motif, 4), False, FULL), "fused_step1": (allsteps.patterns_to_search(motif, 4), False, hiplib.F_STEP1),
             "wide_full": (allsteps.patterns_to_search("CTGTGGGGTCTGGGTG", 14), True, FULL)}
    out = {"lib": os.environ.get("TOPSICLE_HIP_LIB", "in-tree"), "launches": LAUNCHES, "us_per_launch": {}}
    for no_events in (1, 0):
        for name, (pats, wide, flags) in cases.items():
            with hiplib.HipScanner(0) as sc:
                sc.debug_option("no_events", no_events)
                (sc.set_patterns_wide if wide else sc.set_patterns)(pats)
                sc.upload(0, bases, offsets)
                prm = hiplib.make_params(min_len=1000, min_count=mc, window=100, slide=6, trimfirst=100, maxlen=20000, flags=flags)
                for _ in range(600):                              # plan, buffers, the event pool's first steps
                    sc.scan(0, prm)
                sc.sync()
                rounds = []
                for _ in range(ROUNDS):
                    sc.kernel_time_reset()                        # (keeps the window short: the pool of 16 384 pairs still wraps once)
                    t0 = time.perf_counter()
                    for _ in range(LAUNCHES):
                        sc.scan(0, prm)
                    sc.sync()
                    rounds.append(round((time.perf_counter() - t0) / LAUNCHES * 1e6, 4))
                out["us_per_launch"][f"{name}_no_events{no_events}"] = rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
