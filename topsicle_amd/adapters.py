"""Adapters at the telomere end of a read (`--adapters`; HipScanner.adapter_find, tps_batch_adapter_find).

Every length the CLI reports is a position in the telomere-first string, measured from its base 0.  A ligation adapter with its
barcode, or a telomere-capture adapter that sits directly on the first repeat, lies in front of the tract; a read that broke inside
the tract carries none.  The kernel searches the given sequences approximately -- unit-cost edit distance, through nanopore error
rates -- in the first `--adaptersearch` bases of every read with a stored boundary and returns, per pattern, the smallest distance
and the end of the best occurrence.  This module holds what the host adds: the patterns as the library takes them, the naming rule,
the two CSV files and the summary for the log.

The naming rule.  thr_j = floor(err * m_j) and slack_j = thr_j - dist_j.  The best pattern has the largest slack (ties: the
smallest j), the runner is the best of the others.  A read is NAMED when slack_best >= 0 and, with more than one pattern,
slack_best - slack_runner >= margin.  For patterns of one length: "within floor(err m) edits, and no other pattern within `margin`
edits of it".

Patterns are given in the orientation of the telomere-first string: what stands in front of the C-strand repeats of a read whose
telomere is at its start.  The same list is searched on reads whose telomere is at their end, on their reverse complement.
"""
from __future__ import annotations

import math
import os

import numpy as np

from . import analyses
from .analyses import median_cell, write_csv  # noqa: F401  (write_csv stays importable from here)

LETTERS = "ACTG"                  # the packed batch's 2-bit codes
MIN_LEN, MAX_LEN, MAX_PATTERNS, MAX_REGION = 12, 64, 64, 1024
SEARCH_RANGE = (16, MAX_REGION)
DEFAULT_SEARCH, DEFAULT_ERR, DEFAULT_MARGIN = 256, 0.2, 2


class AdapterSpec(analyses.BoundaryAnalysis):
    """What batch.Job(adapters=...) carries: the sequences, the letters of the region [0, search) and `sink(recs, res, dist, end)`,
    called by the worker that scanned a batch while that batch is still resident.  search <= maxlen: the region lies inside the
    span packed for the second pass of the two-pass route."""

    def __init__(self, seqs, search: int = DEFAULT_SEARCH, sink=None):
        self.seqs, self.search, self.sink = [s.upper() for s in seqs], int(search), sink
        self.lens = np.array([len(s) for s in self.seqs], np.int32)

    def regions(self, res, prm):
        return search_regions(res, *self.scan_geometry(prm), self.search)

    def empty(self, n):
        """(m_j, 0): the answer of an empty region"""
        return np.tile(self.lens.astype(np.uint16), (n, 1)), np.zeros((n, len(self.lens)), np.uint16)

    def launch(self, eng, slot, tails, begin, end):
        return eng.adapter_find(slot, self.seqs, tails, begin, end)


def pattern_codes(patterns):
    """(codes uint64[P, 2], lens int32[P]): the patterns as the library takes them, letter i in bits [2i, 2i + 1] of the pattern's
    128 bits.  A (codes, lens) pair is handed through as it is; lengths are the library's to refuse, other letters cannot be coded."""
    if isinstance(patterns, tuple) and len(patterns) == 2 and isinstance(patterns[0], np.ndarray):
        return np.ascontiguousarray(patterns[0], np.uint64).reshape(-1, 2), np.ascontiguousarray(patterns[1], np.int32)
    codes = np.zeros((len(patterns), 2), np.uint64)
    for j, p in enumerate(patterns):
        p = p.upper()
        if len(p) > 2 * 32 or any(c not in LETTERS for c in p):
            raise ValueError(f"a pattern must be at most {MAX_LEN} letters of ACGT, not {p!r}")
        for w in range(2):
            codes[j, w] = sum(LETTERS.index(c) << (2 * i) for i, c in enumerate(p[32 * w:32 * w + 32]))
    return codes, np.array([len(p) for p in patterns], np.int32)


def load_patterns(values) -> list[tuple[str, str]]:
    """[(name, sequence)] of `--adapters`: ONE value that names a file is a FASTA / FASTQ of named sequences, anything else is literal
    sequences, named adapter1, adapter2, ...  Sequences are upper-cased; nothing else is checked here (check())."""
    values = list(values)
    if len(values) == 1 and os.path.isfile(values[0]):
        out, name, seq, fastq_line = [], None, [], 0
        with open(values[0]) as f:
            lines = [ln.strip() for ln in f if ln.strip()]
        if lines and lines[0].startswith("@"):
            for i in range(0, len(lines) - 1, 4):
                out.append(((lines[i][1:].split() or [""])[0], lines[i + 1].upper()))
            return out
        for ln in lines:
            if ln.startswith(">"):
                if name is not None:
                    out.append((name, "".join(seq).upper()))
                name, seq = (ln[1:].split() or [""])[0], []
            elif name is not None:
                seq.append(ln)
        if name is not None:
            out.append((name, "".join(seq).upper()))
        return out
    return [(f"adapter{j + 1}", v.upper()) for j, v in enumerate(values)]


def check(pats, search: int, err: float, margin: int, maxlen: int):
    """None, or what `--adapters` needs, in words: before any input file is read."""
    if not (1 <= len(pats) <= MAX_PATTERNS):
        return f"1..{MAX_PATTERNS} sequences, not {len(pats)}"
    for name, seq in pats:
        if not (MIN_LEN <= len(seq) <= MAX_LEN) or any(c not in "ACGT" for c in seq):
            return f"sequences of {MIN_LEN}..{MAX_LEN} letters of ACGT; {name or '(unnamed)'} has {len(seq)} letters" + \
                   ("" if all(c in "ACGT" for c in seq) else ", other letters among them")
    if len({name for name, _ in pats}) != len(pats) or any(not name or name == "none" for name, _ in pats):
        return "sequences with names of their own, none of them empty or 'none'"
    if not (SEARCH_RANGE[0] <= search <= SEARCH_RANGE[1]) or search > maxlen:
        return f"--adaptersearch {SEARCH_RANGE[0]}..{SEARCH_RANGE[1]} and at most --maxlengthtelo, not {search}"
    if not (0.0 <= err < 1.0) or margin < 0:
        return "--adaptererr in [0, 1) and --adaptermargin >= 0"
    return None


def thresholds(lens, err: float):
    """thr_j = floor(err * m_j) (a product that falls short of a whole number by rounding alone, 0.29 * 100, counts as that number)"""
    return np.array([int(math.floor(err * int(m) + 1e-9)) for m in lens], np.int64)


def name_reads(dist, lens, err: float = DEFAULT_ERR, margin: int = DEFAULT_MARGIN):
    """The naming rule on dist uint16[n, P]: (best int64[n], runner int64[n] (-1 with one pattern), named bool[n])."""
    dist = np.asarray(dist).astype(np.int64).reshape(-1, len(lens))
    n, P = dist.shape
    slack = thresholds(lens, err)[None, :] - dist
    best = slack.argmax(axis=1) if n else np.zeros(0, np.int64)
    rows = np.arange(n)
    s_best = slack[rows, best]
    if P == 1:
        return best, np.full(n, -1, np.int64), s_best >= 0
    others = slack.copy()
    others[rows, best] = np.iinfo(np.int64).min
    runner = others.argmax(axis=1)
    return best, runner, (s_best >= 0) & (s_best - slack[rows, runner] >= margin)


def search_regions(res, trimfirst: int, slide: int, maxlen: int, search: int):
    """(begin, end) int32 arrays for a batch's results: [0, search) for every read whose boundary the CLI would store
    (variants.tract_bounds), begin = end = 0 for every other read."""
    from . import variants
    _b, e = variants.tract_bounds(res, trimfirst, slide, maxlen)
    return np.zeros(len(res), np.int32), np.where(e > 0, search, 0).astype(np.int32)


class Collector(analyses.Collector):
    """The sink of one k of a run: (dist, end) per batch.  A row: (file, readID, tail, telo_length, dist row, end row)."""

    def __init__(self, pats, search: int = DEFAULT_SEARCH, err: float = DEFAULT_ERR, margin: int = DEFAULT_MARGIN):
        super().__init__()
        self.names = [name for name, _ in pats]
        self.spec = AdapterSpec([seq for _, seq in pats], search, self)
        self.err, self.margin = float(err), int(margin)

    def keep_row(self, out, i, file, rid, tail, telo, length):
        return file, rid, tail, telo, out[0][i].copy(), out[1][i].copy()

    def finish(self, paths):
        """(read rows, summary rows, stats) of the run: the naming rule on every read's hits."""
        rows = self.rows_in_order(paths)
        lens = self.spec.lens
        P = len(lens)
        dist = np.array([r[4] for r in rows], np.int64).reshape(len(rows), P)
        end = np.array([r[5] for r in rows], np.int64).reshape(len(rows), P)
        best, runner, named = name_reads(dist, lens, self.err, self.margin)
        read_rows, per = [], [[] for _ in range(P + 1)]            # per pattern (the last: none): (tail, dist, end, telo, from)
        for i, (file, rid, tail, telo, _d, _e) in enumerate(rows):
            b, ru = int(best[i]), int(runner[i])
            a_end = int(end[i, b])
            frm = telo - a_end if named[i] and a_end <= telo else ""
            read_rows.append([file, rid, "forward" if tail == 0 else "reverse", telo, self.names[b] if named[i] else "", int(dist[i, b]), a_end,
                              self.names[ru] if ru >= 0 else "", int(dist[i, ru]) if ru >= 0 else "", frm])
            per[b if named[i] else P].append((tail, int(dist[i, b]), a_end, telo, frm))
        summary_rows = []
        for j in range(P + 1):
            got, is_pat = per[j], j < P
            summary_rows.append([self.names[j] if is_pat else "none", int(lens[j]) if is_pat else "", len(got), sum(1 for g in got if g[0] == 0),
                                 sum(1 for g in got if g[0] != 0), median_cell([g[1] for g in got]) if is_pat else "", median_cell([g[2] for g in got]) if is_pat else "",
                                 median_cell([g[3] for g in got]), median_cell([g[4] for g in got if g[4] != ""]) if is_pat else ""])
        stats = {"reads": len(rows), "named": int(named.sum()), "per_pattern": [len(per[j]) for j in range(P)],
                 "end_median": median_cell([int(end[i, best[i]]) for i in np.nonzero(named)[0]])}
        return read_rows, summary_rows, stats


READ_HEADER = ["file", "readID", "tail", "telo_length", "adapter", "dist", "adapter_end", "runner", "runner_dist", "length_from_adapter"]
SUMMARY_HEADER = ["name", "length", "reads", "tail0", "tail1", "dist_median", "adapter_end_median", "telo_median", "from_adapter_median"]


def summary(col: Collector, stats) -> list[str]:
    """Log lines for a run's adapters."""
    P = len(col.names)
    counts = ", ".join(f"{name} {c}" for name, c in zip(col.names, stats["per_pattern"]) if c) or "none"
    return [f"adapters: {P} sequences of {int(col.spec.lens.min())}..{int(col.spec.lens.max())} letters searched in the first {col.spec.search} bases of "
            f"{stats['reads']} reads (err {col.err:g}, margin {col.margin})",
            f"  named: {stats['named']} reads ({counts}); not named: {stats['reads'] - stats['named']}",
            f"  median adapter end of the named reads: {stats['end_median'] if stats['end_median'] != '' else 'n/a'}"]


# ---- the CLI's side (main.ANALYSES)
FLAG = "adapters"
POWER_NOTE = None                 # (the sequences are searched as given: the motif's root plays no part)


def cli_check(args, root: str):
    """(the sequences come from the command line or from their own small file)"""
    return check(load_patterns(args.adapters), args.adaptersearch, args.adaptererr, args.adaptermargin, args.maxlengthtelo)


def cli_collector(args, unit: str, slide: int):
    return Collector(load_patterns(args.adapters), args.adaptersearch, args.adaptererr, args.adaptermargin)


def finish_and_write(args, k, col, filenames, engines):
    """The naming rule once per run and k; writes the two files, yields the log lines."""
    read_rows, summary_rows, stats = col.finish(filenames)
    yield analyses.write_tables(args.outputDir, k, "adapters", [("adapters", READ_HEADER, read_rows), ("adapter_summary", SUMMARY_HEADER, summary_rows)])
    yield from summary(col, stats)
