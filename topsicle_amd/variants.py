"""Variant repeats of the called telomere tract (`--variants`; HipScanner.variant_census, tps_batch_variant_census).

The census counts, for every read with a stored boundary, the positions of its tract that start a canonical repeat of the motif,
the positions that start a repeat with ONE substituted letter -- by place in the motif and letter seen -- and the rest.  This
module holds what the host adds: the unit as the library takes it, its reduction to the primitive root, the names of the classes
in mutation notation (`T4C`: the T at place 4 of the unit read as C), the two CSV files and the summary for the log.

The unit is the motif as `--pattern` gives it (telomere first, C-strand 5'->3'): the census compares the read, or the reverse
complement of a read whose telomere is at its end, against the rotations of that word.  An isolated substituted unit inside
exact repeats adds exactly m to its class, so class count / m is about the number of such units.
"""
from __future__ import annotations

import csv
import logging

import numpy as np

from . import analyses
from .analyses import BoundaryAnalysis

LETTERS = "ACTG"                  # the packed batch's 2-bit codes
MAX_UNIT = 32
DEFAULT_BIN, DEFAULT_BINS = 500, 40


class VariantSpec(BoundaryAnalysis):
    """What batch.Job(variants=...) carries: the primitive unit, the bin width and count of the profile, and `sink(recs, res,
    counts, profile)`, called by the worker that scanned a batch while that batch is still resident.  The tract of a read is
    [trimfirst, boundary) of its telomere-first string (tract_bounds); the profile is one answer per call."""

    per_batch = 1

    def __init__(self, unit: str, bin: int = DEFAULT_BIN, n_bins: int = DEFAULT_BINS, sink=None):
        self.unit, self.bin, self.n_bins, self.sink = primitive_root(unit.upper()), int(bin), int(n_bins), sink

    def regions(self, res, prm):
        return tract_bounds(res, *self.scan_geometry(prm))

    def empty(self, n):
        cols = 2 + 4 * len(self.unit)
        return np.zeros((n, cols), np.uint32), np.zeros((self.n_bins, cols), np.int64)

    def launch(self, eng, slot, tails, begin, end):
        return eng.variant_census(slot, self.unit, tails, begin, end, self.bin, self.n_bins)


def unit_code(unit: str) -> tuple[int, int]:
    """(code, m): the unit as one 64-bit word of 2-bit codes, letter j in bits [2j, 2j + 1], as tps_motif_hit.unit spells it."""
    unit = unit.upper()
    if not unit or len(unit) > MAX_UNIT or any(c not in LETTERS for c in unit):
        raise ValueError(f"the unit must be 1..{MAX_UNIT} letters of ACGT, not {unit!r}")
    return sum(LETTERS.index(c) << (2 * j) for j, c in enumerate(unit)), len(unit)


def code_unit(code: int, m: int) -> str:
    return "".join(LETTERS[(int(code) >> (2 * j)) & 3] for j in range(m))


def primitive_root(unit: str) -> str:
    """The shortest word the unit is a power of (CCCTAACCCTAA -> CCCTAA); the unit itself where there is none."""
    m = len(unit)
    for d in range(1, m):
        if m % d == 0 and unit[:d] * (m // d) == unit:
            return unit[:d]
    return unit


def class_columns(unit: str) -> list[int]:
    """The 3m columns of a counts row that can hold anything, place after place, letters in ACGT order."""
    return [2 + 4 * p + LETTERS.index(c) for p in range(len(unit)) for c in "ACGT" if c != unit[p]]


def class_names(unit: str) -> list[str]:
    """Mutation notation for class_columns(unit): <letter of the unit><1-based place><letter seen>."""
    return [f"{unit[p]}{p + 1}{c}" for p in range(len(unit)) for c in "ACGT" if c != unit[p]]


def split_row(row, unit: str):
    """(positions, canonical, other, [3m class counts]) of one counts / profile row."""
    cls = [int(row[c]) for c in class_columns(unit)]
    n, canon = int(row[0]), int(row[1])
    return n, canon, n - canon - sum(cls), cls


def tract_bounds(res, trimfirst: int, slide: int, maxlen: int):
    """(begin, end) int32 arrays for a batch's results: the tract [trimfirst, boundary) of every read whose boundary the CLI would
    store (0 < boundary <= maxlen, boundary = bkp * slide + trimfirst), begin = end = 0 for every other read."""
    n = len(res)
    bkp = res["bkp"].astype(np.int64)
    boundary = bkp * slide + trimfirst
    ok = (res["pass"] != 0) & (res["n_win"] > 0) & (bkp >= 0) & (boundary > 0) & (boundary <= maxlen)
    begin = np.where(ok, trimfirst, 0).astype(np.int32)
    end = np.where(ok, boundary, 0).astype(np.int32)
    assert len(begin) == n
    return begin, end


class Collector(analyses.Collector):
    """The sink of one k of a run.  The workers hand it every batch's census (in whatever order they finish): the profile is added
    up at once -- exact integers, the order does not matter -- and the rows, (begin, end, counts), wait for the run's consumer."""

    def __init__(self, unit: str, bin: int = DEFAULT_BIN, n_bins: int = DEFAULT_BINS, trimfirst: int = 100, slide: int = 6, maxlen: int = 20000):
        super().__init__()
        self.spec = VariantSpec(unit, bin, n_bins, self)
        self.unit = self.spec.unit
        self.trimfirst, self.slide, self.maxlen = int(trimfirst), int(slide), int(maxlen)
        cols = 2 + 4 * len(self.unit)
        self.profile = np.zeros((self.spec.n_bins, cols), np.int64)
        self.total = np.zeros(cols, np.int64)
        self.n_tracts = 0

    def __call__(self, recs, res, counts, profile):
        begin, end = tract_bounds(res, self.trimfirst, self.slide, self.maxlen)
        with self._lock:
            self.profile += profile
            self.total += counts.sum(axis=0, dtype=np.int64)
            self.n_tracts += int((end > 0).sum())
            self._pending[id(recs)] = (begin, end, counts)

    def keep_row(self, out, i, file, rid, tail, telo, length):
        begin, end, counts = out
        return file, rid, tail, int(begin[i]), int(end[i]), counts[i]


def read_row(unit: str, filename: str, read_id: str, tail: int, begin: int, end: int, row):
    n, canon, other, cls = split_row(row, unit)
    return [filename, read_id, "forward" if tail == 0 else "reverse", begin, end, n, canon, other] + cls


READ_HEADER = ["file", "readID", "tail", "tract_begin", "tract_end", "positions", "canonical", "other"]
PROFILE_HEADER = ["bin_start", "positions", "canonical", "other"]


def write_reads_csv(path, unit: str, rows):
    """variants_{k}.csv: `rows` = iterable of (file, readID, tail, begin, end, counts row), one per read with a stored boundary."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(READ_HEADER + class_names(unit))
        for r in rows:
            w.writerow(read_row(unit, *r))


def write_profile_csv(path, unit: str, profile, bin: int):
    """variant_profile_{k}.csv: one row per bin, bin_start = its distance back from the boundary."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(PROFILE_HEADER + class_names(unit))
        for b, row in enumerate(profile):
            n, canon, other, cls = split_row(row, unit)
            w.writerow([b * bin, n, canon, other] + cls)


def summary(unit: str, total, n_reads: int, top: int = 5) -> list[str]:
    """Five log lines for the summed counts row `total` of `n_reads` tracts."""
    m = len(unit)
    n, canon, other, cls = split_row(total, unit)
    share = lambda x: 100.0 * x / n if n else 0.0      # noqa: E731
    order = sorted(range(len(cls)), key=lambda i: (-cls[i], i))[:top]
    names = class_names(unit)
    tops = ", ".join(f"{names[i]} {share(cls[i]):.2f}% (~{cls[i] / m:.0f} units)" for i in order if cls[i]) or "none"
    return [f"variant census of {n_reads} tracts against {unit} ({m} letters): {n} positions examined",
            f"  canonical: {canon} positions, {share(canon):.2f}% (~{canon / m:.0f} units)",
            f"  variant (one substituted letter): {sum(cls)} positions, {share(sum(cls)):.2f}%",
            f"  top classes: {tops}",
            f"  other (indels, several changes, not ACGT): {other} positions, {share(other):.2f}%"]


# ---- the CLI's side (main.ANALYSES)
FLAG = "variants"
POWER_NOTE = "the census counts against {unit}"


def cli_check(args, root: str):
    from . import hiplib
    lo, hi = hiplib.VARIANT_BIN_RANGE
    if not (2 <= len(root) <= hiplib.VARIANT_MAX_UNIT) or not (lo <= args.variantbin <= hi) or not (1 <= args.variantbins <= hiplib.VARIANT_MAX_BINS):
        return f"a motif whose root has 2..{hiplib.VARIANT_MAX_UNIT} letters, --variantbin {lo}..{hi} and --variantbins 1..{hiplib.VARIANT_MAX_BINS}"
    return None


def cli_collector(args, unit: str, slide: int):
    return Collector(unit, args.variantbin, args.variantbins, args.trimfirst, slide, args.maxlengthtelo)


def finish_and_write(args, k, col, filenames, engines):
    """The two files of one k; yields the log lines."""
    names = f"{args.outputDir}/variants_{k}.csv", f"{args.outputDir}/variant_profile_{k}.csv"
    write_reads_csv(names[0], col.unit, col.rows_in_order(filenames))
    write_profile_csv(names[1], col.unit, col.profile, col.spec.bin)
    yield f"variant repeats (k = {k}): {names[0]}, {names[1]}"
    yield from summary(col.unit, col.total, col.n_tracts)


def log_summary(unit: str, total, n_reads: int):
    for line in summary(unit, total, n_reads):
        logging.info("%s", line)
