"""The tract map (`--tracts`; HipScanner.tract_map, tps_batch_tract_map): where in the WHOLE read telomere repeats lie, and on which
strand.

The scan measures a telomere at the end of a read it was told to look at.  The map looks at every position of every read instead:
blocks of the read that hold enough near-repeats of the motif are flagged, runs of flagged blocks are tracts, per strand -- C (the
motif as `--pattern` gives it, what a read's head shows) and G (its reverse complement, what a read's tail shows).  The rule is in
include/topsicle_hip.h.  This module holds what the host adds: the defaults, the parameter check, the class of a read from its
tracts, the two CSV files and the summary for the log.  The map only reports: which reads the scan measures does not change.
"""
from __future__ import annotations

import logging

import numpy as np

from . import analyses, variants
from .analyses import write_csv

DEFAULT_BLOCK, DEFAULT_MIN_HITS, DEFAULT_GAP, DEFAULT_MIN_BLOCKS, DEFAULT_MAX_TRACTS, DEFAULT_EDGE = 64, 20, 1, 2, 8, 256
MIN_UNIT, MAX_UNIT = 4, 32
MAX_WORD = 8                      # a hit compares min(m, 8) letters
CLASSES = ("fusion", "both_ends", "interstitial", "terminal", "none")
STRANDS = "CG"


def check(unit: str, block: int, min_hits: int, gap: int, min_blocks: int, max_tracts: int = DEFAULT_MAX_TRACTS, edge: int = DEFAULT_EDGE):
    """None, or what is wrong with the unit (already reduced to its root) or a parameter -- the ranges tps_batch_tract_map takes."""
    if not (MIN_UNIT <= len(unit) <= MAX_UNIT) or any(c not in "ACGT" for c in unit):
        return f"a motif of ACGT whose root has {MIN_UNIT}..{MAX_UNIT} letters (the root of this one is {unit!r})"
    if not (64 <= block <= 1024) or block % 64:
        return "--tractblock a multiple of 64 in 64..1024"
    if not (1 <= min_hits <= block):
        return "--tractminhits 1..tractblock"
    if not (0 <= gap <= 64):
        return "--tractgap 0..64"
    if not (1 <= min_blocks <= 64):
        return "--tractminblocks 1..64"
    if not (1 <= max_tracts <= 16):
        return "at most 1..16 tracts kept per strand"
    if edge < 0:
        return "--tractedge 0 or more"
    return None


class TractSpec:
    """What batch.Job(tracts=...) carries: the primitive unit, the rule's parameters, and `sink(recs, tracts, found, totals)`, called
    by the worker that scanned a batch while that batch is still resident."""

    def __init__(self, unit: str, block: int = DEFAULT_BLOCK, min_hits: int = DEFAULT_MIN_HITS, gap: int = DEFAULT_GAP,
                 min_blocks: int = DEFAULT_MIN_BLOCKS, max_tracts: int = DEFAULT_MAX_TRACTS, sink=None):
        self.unit = variants.primitive_root(unit.upper())
        self.block, self.min_hits, self.gap, self.min_blocks, self.max_tracts = int(block), int(min_hits), int(gap), int(min_blocks), int(max_tracts)
        self.sink = sink

    def kw(self):
        return dict(block=self.block, min_hits=self.min_hits, gap=self.gap, min_blocks=self.min_blocks, max_tracts=self.max_tracts)

    @property
    def slack(self):
        """How far two tracts that abut can overlap in their coordinates: a tract's ends are block edges, and the block that holds
        the junction of a G tract and a C tract can be flagged on both strands."""
        return self.block + min(len(self.unit), MAX_WORD) - 1


def classify(L: int, tracts_C, tracts_G, edge: int = DEFAULT_EDGE, slack: int = 0) -> str:
    """The class of a read of L bases from its tracts, (begin, end, ...) each; the first that applies:
      fusion        some G tract's end and some C tract's begin satisfy -slack <= begin_C - end_G <= edge: G runs into C, head to head;
      both_ends     a C tract with begin <= edge and a G tract with end >= L - edge;
      interstitial  any tract that is neither a C tract with begin <= edge nor a G tract with end >= L - edge;
      terminal      everything else that has a tract;
      none          no tract.
    slack = 0 is the rule on exact coordinates.  The map's coordinates are block edges, so the CLI passes TractSpec.slack: a G tract
    that runs straight into a C tract ends up to block + w - 1 bases BEHIND the C tract's begin."""
    for g in tracts_G:
        for c in tracts_C:
            if -slack <= int(c[0]) - int(g[1]) <= edge:
                return "fusion"
    head = [c for c in tracts_C if int(c[0]) <= edge]
    tail = [g for g in tracts_G if int(g[1]) >= L - edge]
    if head and tail:
        return "both_ends"
    if len(head) < len(tracts_C) or len(tail) < len(tracts_G):
        return "interstitial"
    if head or tail:
        return "terminal"
    return "none"


class Collector(analyses.Collector):
    """The sink of a run: (tracts, found, totals) per batch; the consumer hands every batch back as rows with add_batch."""

    def __init__(self, unit: str, block: int = DEFAULT_BLOCK, min_hits: int = DEFAULT_MIN_HITS, gap: int = DEFAULT_GAP,
                 min_blocks: int = DEFAULT_MIN_BLOCKS, max_tracts: int = DEFAULT_MAX_TRACTS, edge: int = DEFAULT_EDGE):
        super().__init__()                # (_file_rows: input path -> (tract rows, read rows), each file's in read order)
        self.spec = TractSpec(unit, block, min_hits, gap, min_blocks, max_tracts, self)
        self.unit, self.edge = self.spec.unit, int(edge)
        self.classes = dict.fromkeys(CLASSES, 0)

    def __call__(self, recs, tracts, found, totals):       # (no scan results in front: the map does not hang on them)
        with self._lock:
            self._pending[id(recs)] = (tracts, found, totals)

    def add_batch(self, path, file_name: str, ids, lens, tracts, found):
        """The rows of one batch of input file `path`, in read order (the file's consumer calls it: its batches arrive in file order;
        several files may be in flight at once).  ids(r) = the read's name."""
        mt = tracts.shape[2]
        with_tract = np.nonzero(found.sum(axis=1) > 0)[0]
        tract_rows, read_rows, classes = [], [], dict.fromkeys(CLASSES, 0)
        classes["none"] = len(found) - len(with_tract)
        for r in with_tract.tolist():
            n_c, n_g = int(found[r, 0]), int(found[r, 1])
            L = int(lens[r])
            per = [[tuple(int(x) for x in t) for t in tracts[r, s, :min(int(found[r, s]), mt)]] for s in (0, 1)]
            cls = classify(L, per[0], per[1], self.edge, self.spec.slack)
            classes[cls] += 1
            rid = ids(r)
            for s in (0, 1):
                tract_rows += [[file_name, rid, L, STRANDS[s], b, e, nb, h] for b, e, h, nb in per[s]]
            read_rows.append([file_name, rid, L, n_c, n_g, cls, int(max(n_c, n_g) > mt)])
        with self._lock:
            for c, k in classes.items():
                self.classes[c] += k
            mine = self._file_rows.setdefault(path, ([], []))
            mine[0].extend(tract_rows)
            mine[1].extend(read_rows)

    def rows_in_order(self, paths):
        """(tract rows, read rows) of the run, file after file in the order of `paths`."""
        with self._lock:
            return ([r for p in paths for r in self._file_rows.get(p, ([], []))[0]],
                    [r for p in paths for r in self._file_rows.get(p, ([], []))[1]])


TRACT_HEADER = ["file", "readID", "length", "strand", "begin", "end", "blocks", "hits"]
READ_HEADER = ["file", "readID", "length", "n_C", "n_G", "class", "truncated"]


def write_tracts_csv(path, rows):
    """tracts.csv: one row per tract; strand C = the motif as given, G = its reverse complement; [begin, end) in bases of the read as
    stored.  Of a read with more tracts on a strand than the map keeps, the first ones."""
    write_csv(path, TRACT_HEADER, rows)


def write_reads_csv(path, rows):
    """tract_reads.csv: one row per read with at least one tract; n_C / n_G are the true numbers of tracts, truncated = 1 where a
    strand has more of them than tracts.csv lists."""
    write_csv(path, READ_HEADER, rows)


def summary(unit: str, classes: dict) -> list[str]:
    n = sum(classes.values())
    return [f"tract map of {n} reads against {unit} ({len(unit)} letters), reads per class: " + ", ".join(f"{c} {classes[c]}" for c in CLASSES)]


def log_summary(unit: str, classes: dict):
    for line in summary(unit, classes):
        logging.info("%s", line)


# ---- the CLI's side (main.ANALYSES): one collector for the whole run, the map with the first k's job
FLAG = "tracts"
POWER_NOTE = "the map looks for {unit}"


def cli_check(args, root: str):
    return check(root, args.tractblock, args.tractminhits, args.tractgap, args.tractminblocks, DEFAULT_MAX_TRACTS, args.tractedge)


def cli_collector(args, unit: str, slide=None):
    return Collector(unit, args.tractblock, args.tractminhits, args.tractgap, args.tractminblocks, DEFAULT_MAX_TRACTS, args.tractedge)


def finish_and_write(args, k, col, filenames, engines):
    tract_rows, read_rows = col.rows_in_order(filenames)
    write_tracts_csv(f"{args.outputDir}/tracts.csv", tract_rows)
    write_reads_csv(f"{args.outputDir}/tract_reads.csv", read_rows)
    yield f"tract map: {args.outputDir}/tracts.csv, {args.outputDir}/tract_reads.csv"
    yield from summary(col.unit, col.classes)
