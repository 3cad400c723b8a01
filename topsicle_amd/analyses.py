"""What the read analyses share (variants.py, ends.py, adapters.py, refine.py, methyl.py, tracts.py): the shape of an analysis that runs on the
regions behind the called boundaries of a resident batch (batch.run_analysis makes the calls), the collector between the batch workers
and the run's consumer, and the CSV helpers.  Nothing here knows a particular analysis.

Adding a read analysis touches three places: its own module (a spec, a collector, the CLI hooks listed at main.ANALYSES), the list
main.ANALYSES, and its flags in main.build_parser."""
from __future__ import annotations

import csv
import threading

import numpy as np


class BoundaryAnalysis:
    """What batch.Job(variants=, ends=, adapters=, refine=, methyl=) carries.  batch.run_analysis calls, on the worker that scanned a batch and
    while that batch is still resident:

      regions(res, prm) -> (begin, end, *extra)   int32 arrays over the whole batch; begin = end = 0 for a read without a stored boundary
                                                  (needs_records = True: regions(res, prm, recs), the batch's records as well)
      empty(n)          -> outputs                what n reads with empty regions get, in launch()'s order
      launch(eng, slot, tails, begin, end, *extra) -> outputs    the engine call(s) on the reads resident in `slot`
      sink(recs, res, *outputs)                   the spec's `sink` attribute

    The last `per_batch` outputs are one answer for the whole call, not a row per read: they are never scattered over the batch."""

    per_batch = 0
    needs_records = False
    sink = None

    @staticmethod
    def scan_geometry(prm):
        """(trimfirst, slide, maxlen) of the scan whose boundaries the regions hang on."""
        return int(prm.trimfirst), int(prm.slide), int(prm.maxlen)


class Collector:
    """The sink of one k of a run.  The batch workers hand it every batch's outputs in whatever order they finish; they wait until
    the run's consumer, which sees the batches in file order, asks for them (take_batch), picks what it keeps of every read with a
    stored boundary (keep_row, the analysis's own) and hands those rows back (add_file_rows)."""

    def __init__(self):
        self._pending = {}
        self._file_rows = {}
        self._lock = threading.Lock()

    def __call__(self, recs, res, *outputs):
        with self._lock:
            self._pending[id(recs)] = outputs

    def take(self, recs):
        """The outputs of a batch the consumer has in hand."""
        with self._lock:
            return self._pending.pop(id(recs))

    take_batch = take                  # (what row() is given: an analysis with more to hand over than take() overrides it)

    def add_file_rows(self, path, rows):
        """More rows of one input file, in read order."""
        with self._lock:
            self._file_rows.setdefault(path, []).extend(rows)

    def rows_in_order(self, paths):
        return [r for p in paths for r in self._file_rows.get(p, [])]


def write_csv(path, header, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        w.writerows(rows)


def write_tables(outdir, k, title, tables):
    """[(stem, header, rows)] as <outdir>/<stem>_<k>.csv each; returns the log line that names the files."""
    names = [f"{outdir}/{stem}_{k}.csv" for stem, _header, _rows in tables]
    for name, (_stem, header, rows) in zip(names, tables):
        write_csv(name, header, rows)
    return f"{title} (k = {k}): " + ", ".join(names)


def median_cell(xs):
    """The median as a CSV cell: empty without values, a whole number where it is one."""
    if not len(xs):
        return ""
    m = float(np.median(np.asarray(xs, np.float64)))
    return int(m) if m == int(m) else m
