"""End groups named against a reference (`--ends --endref REF`; HipScanner.place_windows).

`--ends` gives groups of reads, numbered by size: a number that means nothing outside one run.  A reference assembly, or a FASTA of
its subtelomeres, gives every chromosome end a name, a boundary that is the same point of the subtelomere in every run, and a place
for every read with enough subtelomere, grouped or not.  The first and the last maxlengthtelo bases of every record of REF are
scanned like reads, with the run's own table and parameters; a piece whose boundary the scan stores, with the telomere on the piece's
own side, is a REFERENCE END, and its window behind that boundary is extracted like a read's (tps_batch_end_window).  After the last
file ONE call per k places the window of every read of end_reads_{k}.csv on all reference windows at once (tps_window_place: an index
of the reference's k-mers built once, one wave per read).  This module holds what the host adds: the pieces, the naming test, the
length measured to the reference end's boundary, the group's name, the three CSV files and the summary for the log.

Only a report: no other output changes.  The thresholds rest on synthetic, independent subtelomeres, like the defaults of `--ends`
and `--anchor` (README, "Named ends").
"""
from __future__ import annotations

import numpy as np

from . import batch, seqio

DEFAULT_MAX_OCC, DEFAULT_MIN_VOTES, DEFAULT_RATIO = 16, 20, 4      # (the votes are anchor.py's statistic: its thresholds)
MAX_SPAN, MAX_REFS, MAX_OCC, MAX_ROWS = 4096, 1024, 64, 262144

REF_HEADER = ["name", "record", "side", "length", "tail", "boundary", "window_begin", "window_end", "kmers", "indexed", "reads_named", "groups_named"]
READ_HEADER = ["file", "readID", "tail", "telo_length", "end", "name", "offset", "votes", "second", "total", "runner_name", "runner", "ref_length"]
GROUP_HEADER = ["end", "reads", "named", "name", "agree", "other_names", "ref_min", "ref_median", "ref_mean", "ref_max", "called_sd", "ref_sd"]


def check(with_ends: bool, span: int, max_occ: int = DEFAULT_MAX_OCC, min_votes: int = DEFAULT_MIN_VOTES, ratio: int = DEFAULT_RATIO):
    """None, or what is wrong, in words for the command line."""
    if not with_ends:
        return "--ends: the windows of its reads are what is placed"
    if span > MAX_SPAN:
        return f"--endspan of at most {MAX_SPAN}"
    if not (1 <= max_occ <= MAX_OCC):
        return f"--endrefmaxocc 1..{MAX_OCC}"
    if min_votes < 1 or ratio < 0:
        return "--endrefminvotes of at least 1 and --endrefratio of at least 0"
    return None


FLAG = "endref"                   # (main.EARLY_CHECKS; the rest of its CLI side is inside ends.finish_and_write)


def cli_check(args, root: str):
    return check(getattr(args, "ends", False), args.endspan, args.endrefmaxocc, args.endrefminvotes, args.endrefratio)


class Piece:
    """One end of a reference record as stored; scanned like a read (`seq` is all the batch code asks of a record)."""

    def __init__(self, record: str, side: str, seq: str):
        self.name, self.record, self.side, self.seq = f"{record}_{side}", record, side, seq


def pieces(path: str, maxlen: int):
    """The two pieces of every record of the reference: side "head" = the first, "tail" = the last min(L, maxlen) bases."""
    for rec in seqio.read_records(path):
        n = min(len(rec.seq), maxlen)
        yield Piece(rec.id, "head", rec.seq[:n])
        yield Piece(rec.id, "tail", rec.seq[len(rec.seq) - n:])


class RefEnd:
    """One piece of the reference under one k: what ref_ends_{k}.csv lists, and its window's rows where it is a reference end."""

    def __init__(self, name, record, side, length):
        self.name, self.record, self.side, self.length = name, record, side, length
        self.tail = self.boundary = self.begin = self.end = self.kmers = None
        self.usable = self.indexed = False
        self.letters, self.codes, self.keep = 0, None, None


def scan_reference(path: str, engine, jobs, collectors, maxlen: int, min_kmers: int):
    """Scan the reference's pieces on `engine` as one more small input: jobs[n] is the run's job of the n-th k with
    collectors[n].spec as its `ends` (a private ends.Collector with anchor set: no row of it reaches the run's own collectors).
    Returns one list of RefEnd per k, in the reference's order."""
    out = [[] for _ in jobs]
    for recs in batch.record_batches(pieces(path, maxlen)):
        outs = batch.scan_jobs(engine, recs, jobs)
        for n, (col, (res, _sums, _raw, _win_off)) in enumerate(zip(collectors, outs)):
            begin, end, _sketch, kept = col.take(recs)
            codes, keep = col.take_windows(recs)
            for i, c in enumerate(recs):
                e = RefEnd(c.name, c.record, c.side, len(c.seq))
                if res["pass"][i]:
                    e.tail = int(res["tail"][i])
                if end[i] > begin[i] and begin[i] <= e.length:                     # the boundary the CLI would store for a read
                    e.boundary = e.begin = int(begin[i])
                    e.end = int(end[i])
                    e.kmers = int(kept[i])
                    e.usable = e.tail == (0 if c.side == "head" else 1)            # the telomere is on the piece's own side
                    e.indexed = e.usable and e.kmers >= min_kmers
                    if e.indexed:
                        e.letters, e.codes, e.keep = max(0, min(e.end, e.length) - e.begin), codes[i].copy(), keep[i].copy()
                out[n].append(e)
    return out


def named_reads(ref, votes, second, min_votes: int = DEFAULT_MIN_VOTES, ratio: int = DEFAULT_RATIO):
    """bool[n]: a read is named when it has a reference row, votes >= min_votes and votes >= ratio * second.  (The runner-up ROW
    does not gate the name: a paralogous end may draw most of the winner's total and still lose every diagonal.)"""
    ref, votes, second = (np.asarray(a, np.int64) for a in (ref, votes, second))
    return (ref >= 0) & (votes >= min_votes) & (votes >= ratio * second)


def group_name(names):
    """(name, agree, other_names) of a group from its named members' reference rows: the row most of them carry, ties to the
    reference end listed first; how many carry it; how many other rows occur.  (None, 0, 0) without a named member."""
    names = np.asarray(names, np.int64)
    if not len(names):
        return None, 0, 0
    rows, counts = np.unique(names, return_counts=True)
    top = int(np.argmax(counts))                       # (argmax: the first of equal maxima = the smallest row)
    return int(rows[top]), int(counts[top]), len(rows) - 1


def _sd(x):
    return float(np.std(x, ddof=1)) if len(x) > 1 else 0.0


def run(rows, read_rows, ref_ends, engine, k: int, span: int, min_kmers: int, max_occ: int = DEFAULT_MAX_OCC, min_votes: int = DEFAULT_MIN_VOTES,
        ratio: int = DEFAULT_RATIO):
    """Name a run.  `rows`: ends.Collector.rows_in_order of a collector that keeps the windows; `read_rows`: the rows of
    end_reads_{k}.csv that Collector.finish made of them; `ref_ends`: scan_reference's list for this k; `engine`: anything with
    place_windows.  Returns (rows of ref_ends_{k}.csv, of named_reads_{k}.csv, of named_ends_{k}.csv, stats for the log)."""
    n = len(rows)
    index = [e for e in ref_ends if e.indexed]
    placed = np.array([i for i, r in enumerate(rows) if r[6] >= min_kmers], np.int64)
    out = np.zeros((7, n), np.int32)
    out[0], out[2] = -1, -1
    if len(index) and len(placed):
        ref_codes = np.stack([e.codes for e in index]).astype(np.uint32)
        ref_keep = np.stack([e.keep for e in index]).astype(np.uint32)
        ref_length = np.array([e.letters for e in index], np.int32)
        for lo in range(0, len(placed), MAX_ROWS):     # (one call for every run the links take: they hold as many reads at the most)
            part = placed[lo:lo + MAX_ROWS]
            codes = np.stack([rows[i][9] for i in part]).astype(np.uint32)
            keep = np.stack([rows[i][10] for i in part]).astype(np.uint32)
            length = np.array([rows[i][8] for i in part], np.int32)
            out[:, part] = engine.place_windows(codes, keep, length, ref_codes, ref_keep, ref_length, span, k, max_occ)
    ref, total, runner_ref, runner, offset, votes, second = out
    was_placed = np.zeros(n, bool)
    was_placed[placed] = bool(len(index))
    named = named_reads(ref, votes, second, min_votes, ratio) & was_placed
    end = np.array([r[7] for r in read_rows], np.int64).reshape(n)
    telo = np.array([r[3] for r in rows], np.int64).reshape(n)
    ref_length_of = telo - offset
    out_reads = []
    for i, r in enumerate(rows):
        row = [r[0], r[1], "forward" if r[2] == 0 else "reverse", r[3], int(end[i])]
        if not was_placed[i]:
            row += [""] * 8
        else:
            row += [index[ref[i]].name if named[i] else "", int(offset[i]), int(votes[i]), int(second[i]), int(total[i]),
                    index[runner_ref[i]].name if runner_ref[i] >= 0 else "", int(runner[i]), int(ref_length_of[i]) if named[i] else ""]
        out_reads.append(row)
    reads_named, groups_named = np.zeros(len(index), np.int64), np.zeros(len(index), np.int64)
    np.add.at(reads_named, ref[named], 1)
    out_groups = []
    split = 0
    for g in range(1, int(end.max()) + 1 if n else 1):
        mem = np.nonzero(end == g)[0]
        nam = mem[named[mem]]
        top, agree, others = group_name(ref[nam])
        row = [g, len(mem), len(nam), "" if top is None else index[top].name, agree, others]
        if top is not None:
            groups_named[top] += 1
            split += others > 0
            ag = nam[ref[nam] == top]
            a = ref_length_of[ag].astype(np.float64)
            row += [int(a.min()), "%.1f" % np.median(a), "%.1f" % a.mean(), int(a.max()), "%.1f" % _sd(telo[ag].astype(np.float64)), "%.1f" % _sd(a)]
        else:
            row += [""] * 6
        out_groups.append(row)
    where = {id(e): j for j, e in enumerate(index)}
    out_refs = []
    for e in ref_ends:
        j = where.get(id(e))
        tail = "" if e.tail is None else "forward" if e.tail == 0 else "reverse"
        stored = e.boundary is not None
        out_refs.append([e.name, e.record, e.side, e.length, tail] + ([e.boundary, e.begin, e.end, e.kmers] if stored else [""] * 4) +
                        [int(e.indexed), 0 if j is None else int(reads_named[j]), 0 if j is None else int(groups_named[j])])
    stats = dict(listed=len(ref_ends), usable=sum(e.usable for e in ref_ends), indexed=len(index), placed=int(was_placed.sum()), named=int(named.sum()),
                 groups=len(out_groups), groups_named=sum(1 for r in out_groups if r[3] != ""), split=int(split),
                 close=int((named & (2 * runner.astype(np.int64) >= total)).sum()), named_lone=int((named & (end == 0)).sum()))
    return out_refs, out_reads, out_groups, stats


def summary(stats, min_kmers: int, min_votes: int, ratio: int) -> list[str]:
    """The log lines of one k."""
    s = stats
    return [f"named ends: {s['usable']} of {s['listed']} reference pieces are ends (a stored boundary, the telomere on the piece's own side), "
            f"{s['indexed']} of them with at least {min_kmers} subtelomere k-mers indexed",
            f"  {s['named']} of {s['placed']} placed reads named (at least {min_votes} votes and {ratio} times the runner-up diagonals'), "
            f"{s['named_lone']} of them without a group (end 0)",
            f"  {s['groups_named']} of {s['groups']} end groups named, {s['split']} with more than one name",
            f"  {s['close']} named reads with a close runner-up (at least half the winner's k-mers): paralogous ends"]
