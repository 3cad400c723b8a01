"""Telomeric reads grouped by chromosome end (`--ends`; HipScanner.end_sketch, HipScanner.sketch_links).

The subtelomere just behind a read's called boundary is the only part of a telomeric read that says which end it came from: reads
of one end share it, reads of different ends mostly do not.  Per read with a stored boundary the batch worker sketches the window
[boundary, min(boundary + span, maxlengthtelo)) of the telomere-first string while the batch is resident -- the smallest hash per
bucket over the k-mers that hold no word of the telomere repeat (tps_batch_end_sketch) -- and after the last file ONE call compares
all sketches with each other (tps_sketch_links).  This module holds what the host adds: the windows, the collector, the groups
(connected components of the links, by union-find), the two CSV files and the summary for the log.

What comes out are GROUPS OF READS, numbered by size -- not chromosome names: no reference is read (endref.py names them against one).  The defaults rest on synthetic,
independent subtelomeres (README, "End groups").
"""
from __future__ import annotations

import numpy as np

from . import analyses, variants
from .analyses import write_csv  # noqa: F401  (stays importable from here)

DEFAULT_SPAN, DEFAULT_K, DEFAULT_BUCKETS, DEFAULT_MIN_MATCH, DEFAULT_MIN_KMERS, DEFAULT_MIN_READS = 2000, 12, 256, 6, 200, 3
DEFAULT_MAX_LINKS = 64            # links kept per sketch (the smallest partners); rows with more are counted in the log
UNIT_RANGE, K_RANGE, BUCKETS, MAX_WINDOW, MAX_SKETCHES, MAX_LINKS = (4, 32), (8, 16), (64, 128, 256, 512), 16384, 262144, 256
EMPTY = 0xFFFFFFFF


def check(unit: str, span: int = DEFAULT_SPAN, k: int = DEFAULT_K, buckets: int = DEFAULT_BUCKETS, min_match: int = DEFAULT_MIN_MATCH,
          min_kmers: int = DEFAULT_MIN_KMERS, min_reads: int = DEFAULT_MIN_READS):
    """None, or what is wrong with the unit (a primitive root) or a value, in words for the command line."""
    if not (UNIT_RANGE[0] <= len(unit) <= UNIT_RANGE[1]) or any(c not in "ACGT" for c in unit.upper()):
        return f"a motif of ACGT whose primitive root has {UNIT_RANGE[0]}..{UNIT_RANGE[1]} letters, not {unit!r}"
    if not (K_RANGE[0] <= k <= K_RANGE[1]):
        return f"--endk {K_RANGE[0]}..{K_RANGE[1]}"
    if buckets not in BUCKETS:
        return "--endbuckets 64, 128, 256 or 512"
    if not (k <= span <= MAX_WINDOW):
        return f"--endspan --endk..{MAX_WINDOW}"
    if not (1 <= min_match <= buckets):
        return "--endminmatch 1..--endbuckets"
    if min_kmers < 1 or min_reads < 1:
        return "--endminkmers and --endminreads of at least 1"
    return None


class EndSpec(analyses.BoundaryAnalysis):
    """What batch.Job(ends=...) carries: the primitive unit, k, the buckets, the window's span, and `sink(recs, res, sketch, kept)`,
    called by the worker that scanned a batch while that batch is still resident.  The window of a read is [boundary, min(boundary +
    span, maxlen)) of its telomere-first string (windows).  `anchor` (anchor.py): the worker also extracts the windows themselves,
    position by position and right behind the sketch, and calls `sink(recs, res, sketch, kept, codes, keep)`."""

    def __init__(self, unit: str, k: int = DEFAULT_K, buckets: int = DEFAULT_BUCKETS, span: int = DEFAULT_SPAN, sink=None, anchor: bool = False):
        self.unit, self.k, self.buckets, self.span, self.sink = variants.primitive_root(unit.upper()), int(k), int(buckets), int(span), sink
        self.anchor = bool(anchor)

    def regions(self, res, prm):
        return windows(res, *self.scan_geometry(prm), self.span)

    def empty(self, n):
        out = np.full((n, self.buckets), EMPTY, np.uint32), np.zeros(n, np.uint32)
        if self.anchor:
            out += np.zeros((n, (self.span + 15) // 16), np.uint32), np.zeros((n, (self.span + 31) // 32), np.uint32)
        return out

    def launch(self, eng, slot, tails, begin, end):
        out = tuple(eng.end_sketch(slot, self.unit, tails, begin, end, self.k, self.buckets))
        if self.anchor:
            out += tuple(eng.end_window(slot, self.unit, tails, begin, end, self.k, self.span))
        return out


def windows(res, trimfirst: int, slide: int, maxlen: int, span: int):
    """(begin, end) int32 arrays for a batch's results: the window [boundary, min(boundary + span, maxlen)) of every read whose
    boundary the CLI would store (variants.tract_bounds), begin = end = 0 for every other read.  The clamp to maxlen is what makes
    one pass and two passes agree: the second pass holds only the first / last min(L, maxlen) bases of a read."""
    _, boundary = variants.tract_bounds(res, trimfirst, slide, maxlen)
    ok = boundary > 0
    b64 = boundary.astype(np.int64)
    begin = np.where(ok, b64, 0).astype(np.int32)
    end = np.where(ok, np.minimum(b64 + span, maxlen), 0).astype(np.int32)
    return begin, end


class UnionFind:
    def __init__(self, n: int):
        self.parent = list(range(n))

    def find(self, x: int) -> int:
        p = self.parent
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def union(self, a: int, b: int):
        ra, rb = self.find(a), self.find(b)
        if ra != rb:
            self.parent[max(ra, rb)] = min(ra, rb)         # the root is the component's first member


def group(n: int, links, min_reads: int = DEFAULT_MIN_READS):
    """end int32[n] from the links of sketch_links (row i: its partners j > i, -1 behind them): connected components, numbered
    1, 2, ... by size, largest first, ties to the component whose first member comes first; 0 = in a component of fewer than
    min_reads members."""
    uf = UnionFind(n)
    ii, pp = np.nonzero(np.asarray(links) >= 0)
    for i, j in zip(ii.tolist(), np.asarray(links)[ii, pp].tolist()):
        uf.union(i, j)
    roots = np.array([uf.find(i) for i in range(n)], np.int64)
    end = np.zeros(n, np.int32)
    if n == 0:
        return end
    first, size = np.unique(roots, return_counts=True)     # (a root is its component's first member)
    order = sorted((int(-s), int(f)) for f, s in zip(first, size) if s >= min_reads)
    for g, (_s, f) in enumerate(order):
        end[roots == f] = g + 1
    return end


def edge_stats(n: int, links, matches):
    """(edges at each row, both directions; its best match) from the links as stored."""
    links, matches = np.asarray(links), np.asarray(matches)
    n_edges = np.zeros(n, np.int64)
    best = np.zeros(n, np.int64)
    ii, pp = np.nonzero(links >= 0)
    jj, mm = links[ii, pp], matches[ii, pp]
    np.add.at(n_edges, ii, 1)
    np.add.at(n_edges, jj, 1)
    np.maximum.at(best, ii, mm)
    np.maximum.at(best, jj, mm)
    return n_edges, best


class Collector(analyses.Collector):
    """The sink of one k of a run: take(recs) gives (begin, end, sketch, kept) of a batch, take_windows(recs) the windows' packed rows
    of the same batch.  finish() links and groups the whole run.  A row: (file, readID, tail, telo_length, begin, end, kept, sketch
    row) -- with anchor followed by (letters of the window, its codes row, its keep row), which anchor.run reads."""

    def __init__(self, unit: str, k: int = DEFAULT_K, buckets: int = DEFAULT_BUCKETS, span: int = DEFAULT_SPAN, min_match: int = DEFAULT_MIN_MATCH,
                 min_kmers: int = DEFAULT_MIN_KMERS, min_reads: int = DEFAULT_MIN_READS, trimfirst: int = 100, slide: int = 6, maxlen: int = 20000,
                 max_links: int = DEFAULT_MAX_LINKS, anchor: bool = False):
        self.spec = EndSpec(unit, k, buckets, span, self, anchor)
        self.unit = self.spec.unit
        self.min_match, self.min_kmers, self.min_reads, self.max_links = int(min_match), int(min_kmers), int(min_reads), int(max_links)
        self.trimfirst, self.slide, self.maxlen = int(trimfirst), int(slide), int(maxlen)
        super().__init__()
        self._pending_windows = {}    # (with anchor: the windows' packed rows of the same batches)
        self.ref_ends = None          # (--endref: endref.scan_reference's list for this k, once the reference has been scanned)

    def __call__(self, recs, res, sketch, kept, codes=None, keep=None):
        begin, end = windows(res, self.trimfirst, self.slide, self.maxlen, self.spec.span)
        with self._lock:
            self._pending[id(recs)] = (begin, end, sketch, kept)
            if codes is not None:
                self._pending_windows[id(recs)] = (codes, keep)

    def take_windows(self, recs):
        """(codes, keep) of the same batch, None without anchor."""
        with self._lock:
            return self._pending_windows.pop(id(recs), None)

    def take_batch(self, recs):
        return self.take(recs) + (self.take_windows(recs),)

    def keep_row(self, out, i, file, rid, tail, telo, length):
        begin, end, sketch, kept, win = out
        row = (file, rid, tail, telo, int(begin[i]), int(end[i]), int(kept[i]), sketch[i].copy())
        if win is not None:                        # the letters the window really has: end clamped to the read
            row += (max(0, min(row[5], length) - row[4]), win[0][i].copy(), win[1][i].copy())
        return row

    def finish(self, paths, engine):
        """Link and group the run's reads on `engine` (anything with sketch_links): (read rows for end_reads_{k}.csv, group rows for
        ends_{k}.csv, stats for the log)."""
        rows = self.rows_in_order(paths)
        part = [i for i, r in enumerate(rows) if r[6] >= self.min_kmers]
        n = len(part)
        if n > MAX_SKETCHES:
            raise ValueError(f"--ends: {n} reads to compare, {MAX_SKETCHES} at most")
        end = np.zeros(n, np.int32)
        n_edges, best = np.zeros(n, np.int64), np.zeros(n, np.int64)
        cut = 0
        if n:
            sketch = np.stack([rows[i][7] for i in part]).astype(np.uint32)
            degree, links, matches = engine.sketch_links(sketch, self.min_match, self.max_links)
            cut = int((degree > self.max_links).sum())
            end = group(n, links, self.min_reads)
            n_edges, best = edge_stats(n, links, matches)
        where = {i: p for p, i in enumerate(part)}
        read_rows = []
        for i, (file, rid, tail, telo, b, e, kept) in enumerate(r[:7] for r in rows):
            p = where.get(i)
            read_rows.append([file, rid, "forward" if tail == 0 else "reverse", telo, b, e, kept] +
                             ([0, 0, 0] if p is None else [int(end[p]), int(n_edges[p]), int(best[p])]))
        group_rows = []
        for g in range(1, int(end.max()) + 1 if n else 1):
            mem = [rows[part[p]] for p in np.nonzero(end == g)[0]]
            telo = np.array([r[3] for r in mem], np.float64)
            fwd = sum(1 for r in mem if r[2] == 0)
            group_rows.append([g, len(mem), fwd, len(mem) - fwd, int(telo.min()), "%.1f" % np.median(telo), "%.1f" % telo.mean(), int(telo.max())])
        stats = dict(reads=len(rows), compared=n, groups=len(group_rows), assigned=int((end > 0).sum()), cut=cut)
        return read_rows, group_rows, stats


READ_HEADER = ["file", "readID", "tail", "telo_length", "window_begin", "window_end", "kmers", "end", "links", "best_match"]
GROUP_HEADER = ["end", "reads", "forward", "reverse", "telo_min", "telo_median", "telo_mean", "telo_max"]


def summary(col: Collector, stats) -> list[str]:
    """The log lines of one k."""
    s = stats
    return [f"end groups against {col.unit}: {s['reads']} reads with a boundary, {s['compared']} of them with at least {col.min_kmers} "
            f"subtelomere {col.spec.k}-mers compared",
            f"  {s['groups']} groups of at least {col.min_reads} reads: {s['assigned']} reads assigned, {s['reads'] - s['assigned']} unassigned (end 0)",
            f"  {s['cut']} reads had more than {col.max_links} partners behind them: their links were cut at {col.max_links}"]


# ---- the CLI's side (main.ANALYSES)
FLAG = "ends"
POWER_NOTE = "k-mers with words of {unit} are left out of the sketches"


def cli_check(args, root: str):
    return check(root, args.endspan, args.endk, args.endbuckets, args.endminmatch, args.endminkmers, args.endminreads)


def cli_collector(args, unit: str, slide: int, anchor=None):
    """`anchor`: None = as --anchor or --endref ask (either keeps the windows)."""
    if anchor is None:
        anchor = bool(getattr(args, "anchor", False) or getattr(args, "endref", None))
    return Collector(unit, args.endk, args.endbuckets, args.endspan, args.endminmatch, args.endminkmers, args.endminreads, args.trimfirst, slide,
                     args.maxlengthtelo, anchor=anchor)


def finish_and_write(args, k, col, filenames, engines):
    """All pairs of the run's sketches: one call per k, on one context, after the last file; then, with --anchor, one boundary per
    group -- behind it, with --consensus, one sequence per group -- and, with the ends of --endref's reference (col.ref_ends), one
    name per read.  Writes the files; yields the log lines."""
    from . import anchor, consensus, endref
    out = args.outputDir
    try:
        read_rows, group_rows, stats = col.finish(filenames, engines[0])
    except ValueError as e:                        # more reads than one link call takes: said, not hidden; every other output stands
        yield f"{e}; no end groups written for k = {k}"
        return
    col.read_rows = read_rows                      # (methyl.finish_and_write groups its reads by them)
    yield analyses.write_tables(out, k, "end groups", [("end_reads", READ_HEADER, read_rows), ("ends", GROUP_HEADER, group_rows)])
    yield from summary(col, stats)
    if getattr(args, "anchor", False):
        # every grouped read's window against its group's reference, one call per k
        a_reads, a_groups, a_stats = anchor.run(col.rows_in_order(filenames), read_rows, engines[0], col.spec.k, col.spec.span,
                                                args.anchorminvotes, args.anchorratio)
        yield analyses.write_tables(out, k, "anchored lengths", [("anchored_reads", anchor.READ_HEADER, a_reads), ("anchored_ends", anchor.GROUP_HEADER, a_groups)])
        yield from anchor.summary(a_stats, args.anchorminvotes, args.anchorratio)
        if getattr(args, "consensus", False):
            # every anchored read's window against its group's reference base by base, then against the group's consensus: two calls per k
            records, c_groups, c_reads, references, c_stats = consensus.run(col.rows_in_order(filenames), read_rows, a_reads, a_groups, engines[0], col.unit,
                                                                            col.spec.span, args.consensusmindepth, args.minSeqLength)
            yield analyses.write_tables(out, k, "end consensus", [("end_consensus", consensus.GROUP_HEADER, c_groups), ("consensus_reads", consensus.READ_HEADER, c_reads)])
            consensus.write_fasta(f"{out}/end_consensus_{k}.fa", records)
            consensus.write_fasta(f"{out}/end_reference_{k}.fa", references)
            yield f"end consensus (k = {k}): {out}/end_consensus_{k}.fa, {out}/end_reference_{k}.fa"
            yield from consensus.summary(c_stats, args.consensusmindepth, args.maxlengthtelo)
    if col.ref_ends is not None:
        # every read's window on all the reference's ends, one call per k
        refs, reads, groups, r_stats = endref.run(col.rows_in_order(filenames), read_rows, col.ref_ends, engines[0], col.spec.k, col.spec.span,
                                                  args.endminkmers, args.endrefmaxocc, args.endrefminvotes, args.endrefratio)
        yield analyses.write_tables(out, k, "named ends", [("ref_ends", endref.REF_HEADER, refs), ("named_reads", endref.READ_HEADER, reads),
                                                          ("named_ends", endref.GROUP_HEADER, groups)])
        yield from endref.summary(r_stats, args.endminkmers, args.endrefminvotes, args.endrefratio)
