#!/usr/bin/env python3
"""Kernel time of the wide-table scan (tps_scan_kernel_wide) beside the generic kernel it is measured against.

    scripts/wide_bench.py [--out profiles/<dir>/wide.json] [--baseline-tree OTHER_CHECKOUT] [--reads 10000] [--len 15000]

On 10 000 x 15 kb synthetic reads, sums + change point and again with raw rows, device events (tps_kernel_time_ms), warm-up, at
least 0.5 s timed per arm, the arms of one comparison alternating in ONE process:
  (a) a 15-letter motif at k = 13 (P = 30, a narrow table) on the generic kernel ("force_generic": what such a table ran on before)
      -- with --baseline-tree the same arm on that checkout's package and library too, in the same process (the parent commit's
      build: the baseline is unchanged code);
  (b) the same table through the wide kernel (tps_set_patterns_wide takes narrow tables);
  (c) the 23- and 32-letter motifs at the reference's defaults (k = len - 2, slide = len), and CCCTAA at k = 4 on its own kernel:
      the distance to "a 23-letter motif within 3x of CCCTAA".
Guard (exit status 1 when missed): (b) <= 2 x (a) in both modes -- on identical work the wide kernel differs from the generic
one in building 64- instead of 32-bit codes; beyond 2x the likely cause is windows recounted per pattern.
`--one ARM` runs a single arm for a while (a profiler's target)."""
import argparse
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from topsicle_amd import allsteps, hiplib, synth       # noqa: E402

SUMS = hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS
M15, M23, M32 = "ACGGATGTCTAACTT", "ACGGATGTCTAACTTCTTGGTGT", "ACGGATGTCTAACTTCTTGGTGTACGGATTTG"


def package_of(tree):
    """Another checkout's topsicle_amd (its own binding and its own libtopsicle_hip.so) beside this one, as topsicle_amd_baseline."""
    import importlib
    import importlib.util
    pkg = os.path.join(tree, "topsicle_amd")
    spec = importlib.util.spec_from_file_location("topsicle_amd_baseline", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["topsicle_amd_baseline"] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module("topsicle_amd_baseline.hiplib")


class Arm:
    def __init__(self, name, motif, k, slide, wide, generic=False, binding=None, cutoff=0.2):
        self.name, self.motif, self.k, self.slide, self.wide, self.generic, self.cutoff = name, motif, k, slide, wide, generic, cutoff
        self.binding = binding or hiplib

    def open(self, n_reads, read_len):
        self.sc = self.binding.HipScanner(0)
        if self.generic:
            self.sc.debug_option("force_generic", 1)
        pats = allsteps.patterns_to_search(self.motif, self.k)
        (self.sc.set_patterns_wide if self.wide else self.sc.set_patterns)(pats)
        self.P = len(pats)
        b, o, _ = synth.make_reads(n_reads, read_len, self.motif, 20261016, errors=synth.ONT)
        for s in range(2):
            self.sc.upload(s, b, o)

    def params(self, raw):
        return self.binding.make_params(min_len=9000, min_count=allsteps.min_count_for_cutoff(self.cutoff, 1000 / len(self.motif), 1000),
                                  slide=self.slide, flags=SUMS | (hiplib.F_STORE_RAW if raw else 0))

    def burst(self, raw, launches):
        prm = self.params(raw)
        self.sc.kernel_time_reset()
        for i in range(launches):
            self.sc.scan(i % 2, prm)
        self.sc.sync()
        n, tot, _ = self.sc.kernel_time_ms()
        self.info = self.sc.kernel_info(0)
        self.n_pass = int(self.sc.results(0)["pass"].sum())
        return n, tot


def measure(arms, raw, min_s=0.5):
    """Alternating bursts until every arm has at least min_s of kernel time; -> {arm: dict(us, launches, kernel, passing)}."""
    for a in arms:
        a.burst(raw, 5)                                    # warm-up: plans, buffers, clocks
    tot = {a.name: [0, 0.0] for a in arms}
    while min(t[1] for t in tot.values()) < min_s * 1000.0:
        for a in arms:
            n, ms = a.burst(raw, 20)
            tot[a.name][0] += n
            tot[a.name][1] += ms
    return {a.name: dict(us_per_launch=round(1000.0 * tot[a.name][1] / tot[a.name][0], 2), launches=tot[a.name][0], kernel=a.info.split(" lds=")[0],
                         lds=a.info.split(" lds=")[1], patterns=a.P, k=a.k, slide=a.slide, reads_passing=a.n_pass) for a in arms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--baseline-tree")
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--len", type=int, default=15000)
    ap.add_argument("--one")
    args = ap.parse_args()
    arms = [Arm("a_generic_15", M15, 13, 6, wide=False, generic=True), Arm("b_wide_15", M15, 13, 6, wide=True)]
    if args.baseline_tree:
        arms.append(Arm("a_generic_15_baseline_tree", M15, 13, 6, wide=False, generic=True, binding=package_of(args.baseline_tree)))
    others = [Arm("c_wide_23", M23, 21, 23, wide=True), Arm("c_wide_32", M32, 30, 32, wide=True),
              Arm("c_wide_23_slide6", M23, 21, 6, wide=True), Arm("ccctaa_k4", "CCCTAA", 4, 6, wide=False, cutoff=0.7)]
    if args.one:
        arm = next(a for a in arms + others if a.name == args.one)
        arm.open(args.reads, args.len)
        t0 = time.time()
        while time.time() - t0 < 3.0:
            arm.burst(False, 20)
            arm.burst(True, 20)
        print(arm.info)
        return 0
    out = dict(reads=args.reads, read_len=args.len, device=None, modes={})
    for group in (arms, others):
        for a in group:
            a.open(args.reads, args.len)
        out["device"] = group[0].sc.device_info()
        for raw in (False, True):
            out["modes"].setdefault("raw_rows" if raw else "sums", {}).update(measure(group, raw))
        for a in group:
            a.sc.close()
    ok = True
    for mode, r in out["modes"].items():
        ratio = r["b_wide_15"]["us_per_launch"] / r["a_generic_15"]["us_per_launch"]
        r["guard_b_over_a"] = round(ratio, 3)
        r["c23_over_ccctaa"] = round(r["c_wide_23"]["us_per_launch"] / r["ccctaa_k4"]["us_per_launch"], 2)
        ok = ok and ratio <= 2.0
    out["guard_met"] = ok
    text = json.dumps(out, indent=1)
    text = re.sub(r"\{\n\s+(\"us_per_launch\"[^}]*?)\n\s+\}", lambda m: "{" + re.sub(r"\n\s+", " ", m.group(1)) + "}", text)      # one line per arm
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
