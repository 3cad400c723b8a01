"""The boundary at base resolution, and its support (`--refine`; HipScanner.boundary_refine, tps_batch_boundary_refine).

Every length the CLI reports rests on one change point on the window sums: boundary = bkp * slide + trimfirst, on a grid of `slide`
bases under windows of 100, and binary segmentation always returns a split -- nothing says how sharp it was, or whether the read has a
subtelomere at all.  The kernel looks at the same region position by position: every w-letter word of the telomere-first string that
lies within one substitution of the repeat is a hit worth +hit, any other position costs miss, and the boundary is where the running
sum P peaks -- the likelihood of "telomere up to here, something else from here on".  Beside the peak it returns the evidence: how far
P falls from there to the end of the region (`drop`), how much worse the best boundary at least `sep` positions away is (`margin`),
what the called boundary scores (`called_deficit`), and the hit densities on either side.  This module holds what the host adds: the
regions, the class rule, the two CSV files and the summary for the log.

The class rule, first match wins: `no_telomere` score < minscore; `open` drop < mindrop -- the tract runs to the end of what was looked
at, the length is a lower bound; `ambiguous` a runner within minmargin of the score; `clean` everything else.  The thresholds rest on
synthetic reads.
"""
from __future__ import annotations

import numpy as np

from . import analyses
from .analyses import median_cell, write_csv  # noqa: F401  (write_csv stays importable from here)

DEFAULT_HIT, DEFAULT_MISS, DEFAULT_SEP = 2, 1, 200
DEFAULT_MIN_SCORE, DEFAULT_MIN_DROP, DEFAULT_MIN_MARGIN = 100, 100, 50
WEIGHT_RANGE, SEP_RANGE, MAX_REGION = (1, 16), (1, 65535), 65536
UNIT_RANGE = (4, 32)
CLASSES = ("no_telomere", "open", "ambiguous", "clean")


def word_len(unit: str) -> int:
    """w: the letters of the words the kernel looks up"""
    return min(len(unit), 8)


class RefineSpec(analyses.BoundaryAnalysis):
    """What batch.Job(refine=...) carries: the primitive unit, the rule's weights and `sink(recs, res, rows)`, called by the worker
    that scanned a batch while that batch is still resident.  The region ends at maxlen: it lies inside the span packed for the
    second pass of the two-pass route."""

    def __init__(self, unit: str, hit: int = DEFAULT_HIT, miss: int = DEFAULT_MISS, sep: int = DEFAULT_SEP, sink=None):
        self.unit, self.hit, self.miss, self.sep, self.sink = unit.upper(), int(hit), int(miss), int(sep), sink
        self.w = word_len(self.unit)

    def regions(self, res, prm):
        return regions(res, *self.scan_geometry(prm), self.w)

    def empty(self, n):
        """the row of an empty region"""
        from . import hiplib
        rows = np.zeros(n, hiplib.REFINE_DTYPE)
        rows["runner_pos"] = -1
        return rows,

    def launch(self, eng, slot, tails, begin, end, at):
        return eng.boundary_refine(slot, self.unit, tails, begin, end, at, hit=self.hit, miss=self.miss, sep=self.sep),


def check(unit: str, hit: int, miss: int, sep: int, minscore: int, mindrop: int, minmargin: int, trimfirst: int, maxlen: int):
    """None, or what `--refine` needs, in words: before any input file is read."""
    if not (UNIT_RANGE[0] <= len(unit) <= UNIT_RANGE[1]):
        return f"a motif whose root has {UNIT_RANGE[0]}..{UNIT_RANGE[1]} letters, not {len(unit)}"
    if not (WEIGHT_RANGE[0] <= hit <= WEIGHT_RANGE[1]) or not (WEIGHT_RANGE[0] <= miss <= WEIGHT_RANGE[1]):
        return f"--refinehit and --refinemiss in {WEIGHT_RANGE[0]}..{WEIGHT_RANGE[1]}"
    if not (SEP_RANGE[0] <= sep <= SEP_RANGE[1]):
        return f"--refinesep in {SEP_RANGE[0]}..{SEP_RANGE[1]}"
    if minscore < 0 or mindrop < 0 or minmargin < 0:
        return "--refineminscore, --refinemindrop and --refineminmargin >= 0"
    if maxlen - trimfirst > MAX_REGION:
        return f"a region of at most {MAX_REGION} bases: --maxlengthtelo - --trimfirst is {maxlen - trimfirst}"
    return None


def regions(res, trimfirst: int, slide: int, maxlen: int, w: int):
    """(begin, end, at) int32 arrays for a batch's results: for every read whose boundary the CLI would store (variants.tract_bounds)
    the region [trimfirst, maxlen) -- the kernel clamps it to the read -- and at = the position whose word ends where the called
    boundary lies, max(begin, boundary - (w - 1)); begin = end = at = 0 for every other read."""
    from . import variants
    b, e = variants.tract_bounds(res, trimfirst, slide, maxlen)
    ok = e > 0
    begin = np.where(ok, trimfirst, 0).astype(np.int32)
    end = np.where(ok, maxlen, 0).astype(np.int32)
    at = np.where(ok, np.maximum(begin, e.astype(np.int64) - (w - 1)), 0).astype(np.int32)
    return begin, end, at


def refined_length(row, begin: int, w: int) -> int:
    """pos is where the last word of the tract starts + 1: the tract ends w - 1 letters further on; nothing found: begin"""
    pos = int(row["pos"])
    return begin if pos == begin else pos + w - 1


def classify(score: int, drop: int, margin, minscore: int = DEFAULT_MIN_SCORE, mindrop: int = DEFAULT_MIN_DROP, minmargin: int = DEFAULT_MIN_MARGIN) -> str:
    """The class rule; margin = None where there is no runner."""
    if score < minscore:
        return "no_telomere"
    if drop < mindrop:
        return "open"
    if margin is not None and margin < minmargin:
        return "ambiguous"
    return "clean"


class Collector(analyses.Collector):
    """The sink of one k of a run: the kernel's rows per batch.  A row: (file, readID, tail, telo_length, the read's row)."""

    def __init__(self, unit: str, hit: int = DEFAULT_HIT, miss: int = DEFAULT_MISS, sep: int = DEFAULT_SEP, minscore: int = DEFAULT_MIN_SCORE,
                 mindrop: int = DEFAULT_MIN_DROP, minmargin: int = DEFAULT_MIN_MARGIN, trimfirst: int = 100):
        super().__init__()
        self.spec = RefineSpec(unit, hit, miss, sep, self)
        self.minscore, self.mindrop, self.minmargin, self.trimfirst = int(minscore), int(mindrop), int(minmargin), int(trimfirst)

    def keep_row(self, out, i, file, rid, tail, telo, length):
        return file, rid, tail, telo, out[0][i].copy()

    def read_row(self, file, rid, tail, telo, row):
        """One line of refined_{k}.csv and its class."""
        begin, w = self.trimfirst, self.spec.w
        length = refined_length(row, begin, w)
        score, drop = int(row["score"]), int(row["drop"])
        margin = None if int(row["runner_pos"]) < 0 else score - int(row["runner"])
        n_before = int(row["pos"]) - begin
        n_after = score_positions(row, self.spec.hit, self.spec.miss) - n_before
        cls = classify(score, drop, margin, self.minscore, self.mindrop, self.minmargin)
        return [file, rid, "forward" if tail == 0 else "reverse", telo, length, length - telo, score, drop, "" if margin is None else margin,
                score - int(row["at_score"]), _density(int(row["hits_before"]), n_before), _density(int(row["hits_after"]), n_after), cls]

    def finish(self, paths):
        """(read rows, summary rows, stats) of the run."""
        read_rows = [self.read_row(*r) for r in self.rows_in_order(paths)]
        per = {c: [r for r in read_rows if r[-1] == c] for c in CLASSES}
        summary_rows = [[c, len(per[c]), median_cell([r[3] for r in per[c]]), median_cell([r[4] for r in per[c]]), median_cell([abs(r[5]) for r in per[c]])] for c in CLASSES]
        stats = {"reads": len(read_rows), "counts": {c: len(per[c]) for c in CLASSES}, "clean_shift_median": median_cell([abs(r[5]) for r in per["clean"]])}
        return read_rows, summary_rows, stats


def score_positions(row, hit: int, miss: int) -> int:
    """N, the positions of the region, from the row itself: P(begin + N) = score - drop = hit * hits - miss * (N - hits)."""
    hits = int(row["hits_before"]) + int(row["hits_after"])
    return hits + (hit * hits - (int(row["score"]) - int(row["drop"]))) // miss


def _density(hits: int, positions: int) -> str:
    return "" if positions <= 0 else "%.3f" % (hits / positions)


READ_HEADER = ["file", "readID", "tail", "telo_length", "refined_length", "shift", "score", "drop", "margin", "called_deficit", "density_before", "density_after",
               "class"]
SUMMARY_HEADER = ["class", "reads", "telo_median", "refined_median", "abs_shift_median"]


def summary(col: Collector, stats) -> list[str]:
    """Log lines for a run's refined boundaries."""
    s = col.spec
    counts = ", ".join(f"{c} {stats['counts'][c]}" for c in CLASSES)
    med = stats["clean_shift_median"]
    return [f"refined boundaries: {stats['reads']} reads against {s.unit} (hit {s.hit}, miss {s.miss}, sep {s.sep}; "
            f"minscore {col.minscore}, mindrop {col.mindrop}, minmargin {col.minmargin})",
            f"  {counts}",
            f"  median |refined_length - telo_length| of the clean reads: {med if med != '' else 'n/a'}"]


# ---- the CLI's side (main.ANALYSES)
FLAG = "refine"
POWER_NOTE = "the hits are words of {unit}"


def cli_check(args, root: str):
    return check(root, args.refinehit, args.refinemiss, args.refinesep, args.refineminscore, args.refinemindrop, args.refineminmargin,
                 args.trimfirst, args.maxlengthtelo)


def cli_collector(args, unit: str, slide: int):
    return Collector(unit, args.refinehit, args.refinemiss, args.refinesep, args.refineminscore, args.refinemindrop, args.refineminmargin, args.trimfirst)


def finish_and_write(args, k, col, filenames, engines):
    """The class rule once per run and k; writes the two files, yields the log lines."""
    read_rows, summary_rows, stats = col.finish(filenames)
    yield analyses.write_tables(args.outputDir, k, "refined boundaries", [("refined", READ_HEADER, read_rows), ("refine_summary", SUMMARY_HEADER, summary_rows)])
    yield from summary(col, stats)
