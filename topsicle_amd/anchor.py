"""Anchored telomere lengths per chromosome end (`--ends --anchor`; HipScanner.end_window, HipScanner.anchor_offsets).

`--ends` groups telomeric reads by the end they came from; the telomere lengths it then summarises per group are every read's own
change-point call, a few hundred bases of noise each.  Reads of one end share their subtelomere, so the group can serve as its own
reference: the batch worker keeps every read's window behind its boundary position by position (tps_batch_end_window: packed letters
and the sketch's keep bits), and after `ends.Collector.finish` has grouped the run ONE call places every grouped read's window on
the window of its group's reference read by votes on their diagonals (tps_window_offsets).  This module holds what the host adds:
the choice of the reference, the anchoring test, the consensus boundary, the two CSV files and the summary for the log.

Only a report: no other output changes.  The thresholds rest on synthetic, independent subtelomeres, like the defaults of `--ends`
(README, "Anchored lengths").
"""
from __future__ import annotations

import numpy as np

DEFAULT_MIN_VOTES, DEFAULT_RATIO = 20, 4      # (synthetic sets: a read of the reference's end gets >= 187 votes, a runner-up <= 3, a stranger <= 1)
MAX_SPAN = 4096

READ_HEADER = ["file", "readID", "tail", "telo_length", "end", "reference", "offset", "votes", "second", "shift", "anchored_length"]
GROUP_HEADER = ["end", "reads", "anchored", "reference", "consensus_boundary", "anchored_min", "anchored_median", "anchored_mean", "anchored_max",
                "called_sd", "anchored_sd"]


def check(with_ends: bool, span: int, min_votes: int = DEFAULT_MIN_VOTES, ratio: int = DEFAULT_RATIO):
    """None, or what is wrong, in words for the command line."""
    if not with_ends:
        return "--ends: the groups are what the reads are anchored in"
    if span > MAX_SPAN:
        return f"--endspan of at most {MAX_SPAN}"
    if min_votes < 1 or ratio < 0:
        return "--anchorminvotes of at least 1 and --anchorratio of at least 0"
    return None


FLAG = "anchor"                   # (main.EARLY_CHECKS; the rest of its CLI side is inside ends.finish_and_write)


def cli_check(args, root: str):
    return check(getattr(args, "ends", False), args.endspan, args.anchorminvotes, args.anchorratio)


def references(end, links):
    """ref int32[n]: for a read of group end[i] > 0 the member of its group with the most links, the first of them in run order; -1
    for a read without a group."""
    end, links = np.asarray(end, np.int64), np.asarray(links, np.int64)
    ref = np.full(len(end), -1, np.int32)
    for g in np.unique(end[end > 0]):
        mem = np.nonzero(end == g)[0]
        ref[mem] = mem[np.argmax(links[mem])]      # (argmax: the first of equal maxima)
    return ref


def lower_median(x):
    x = np.sort(np.asarray(x))
    return x[(len(x) - 1) // 2]


def anchor_groups(end, ref, begin, offset, votes, second, min_votes: int = DEFAULT_MIN_VOTES, ratio: int = DEFAULT_RATIO):
    """(anchored bool[n], pos int64[n], consensus {group: C}): a read is anchored when votes >= min_votes and votes >= ratio * second;
    pos = its boundary in its reference's coordinates, begin_i + (offset_i + begin_ref - begin_i); C = the lower median of pos over
    the group's anchored members (a group without one has no entry)."""
    end, ref, begin = np.asarray(end, np.int64), np.asarray(ref, np.int64), np.asarray(begin, np.int64)
    offset, votes, second = (np.asarray(a, np.int64) for a in (offset, votes, second))
    anchored = (end > 0) & (ref >= 0) & (votes >= min_votes) & (votes >= ratio * second)
    pos = np.where(anchored, begin + (offset + begin[np.maximum(ref, 0)] - begin), 0)
    consensus = {int(g): int(lower_median(pos[anchored & (end == g)])) for g in np.unique(end[anchored])}
    return anchored, pos, consensus


def _sd(x):
    return float(np.std(x, ddof=1)) if len(x) > 1 else 0.0


def run(rows, read_rows, engine, k: int, span: int, min_votes: int = DEFAULT_MIN_VOTES, ratio: int = DEFAULT_RATIO):
    """Anchor a run.  `rows`: ends.Collector.rows_in_order of a collector with anchor set (file, readID, tail, telo_length, begin, end,
    kept, sketch row, letters, codes row, keep row); `read_rows`: the rows of end_reads_{k}.csv that Collector.finish made of them
    (columns `end` and `links`); `engine`: anything with anchor_offsets.  Returns (rows of anchored_reads_{k}.csv, rows of
    anchored_ends_{k}.csv, stats for the log)."""
    n = len(rows)
    end = np.array([r[7] for r in read_rows], np.int64).reshape(n)
    links = np.array([r[8] for r in read_rows], np.int64).reshape(n)
    begin = np.array([r[4] for r in rows], np.int64).reshape(n)
    telo = [r[3] for r in rows]
    ref = references(end, links)
    offset, votes, second = (np.zeros(n, np.int32) for _ in range(3))
    grouped = np.nonzero(end > 0)[0]
    if len(grouped):
        # the grouped reads of the run in one call (they took part in the links: at most as many as those take)
        where = np.full(n, -1, np.int32)
        where[grouped] = np.arange(len(grouped), dtype=np.int32)
        codes = np.stack([rows[i][9] for i in grouped]).astype(np.uint32)
        keep = np.stack([rows[i][10] for i in grouped]).astype(np.uint32)
        length = np.array([rows[i][8] for i in grouped], np.int32)
        offset[grouped], votes[grouped], second[grouped] = engine.anchor_offsets(codes, keep, length, where[ref[grouped]], span, k)
    anchored, pos, consensus = anchor_groups(end, ref, begin, offset, votes, second, min_votes, ratio)
    shift = np.zeros(n, np.int64)
    out_reads = []
    for i, r in enumerate(rows):
        row = [r[0], r[1], "forward" if r[2] == 0 else "reverse", r[3], int(end[i]), rows[ref[i]][1] if ref[i] >= 0 else ""]
        if anchored[i]:
            shift[i] = consensus[int(end[i])] - pos[i]
            row += [int(offset[i]), int(votes[i]), int(second[i]), int(shift[i]), telo[i] + int(shift[i])]
        else:
            row += [""] * 5
        out_reads.append(row)
    out_groups = []
    for g in range(1, int(end.max()) + 1 if n else 1):
        mem = np.nonzero(end == g)[0]
        anc = mem[anchored[mem]]
        row = [g, len(mem), len(anc), rows[ref[mem[0]]][1]]
        if len(anc):
            called = np.array([telo[i] for i in anc], np.float64)
            a = called + shift[anc]
            row += [consensus[g], int(a.min()), "%.1f" % np.median(a), "%.1f" % a.mean(), int(a.max()), "%.1f" % _sd(called), "%.1f" % _sd(a)]
        else:
            row += [""] * 7
        out_groups.append(row)
    n_anchored = int(anchored.sum())
    stats = dict(groups=len(out_groups), grouped=len(grouped), anchored=n_anchored,
                 median_shift=float(np.median(np.abs(shift[anchored]))) if n_anchored else 0.0)
    return out_reads, out_groups, stats


def summary(stats, min_votes: int, ratio: int) -> list[str]:
    """The log lines of one k."""
    s = stats
    return [f"anchored lengths: {s['groups']} end groups, every read placed on its group's reference read (the member with the most links)",
            f"  {s['anchored']} of {s['grouped']} grouped reads anchored (at least {min_votes} votes and {ratio} times the runner-up's), "
            f"{s['grouped'] - s['anchored']} not",
            f"  median |shift| of a called boundary against its group's consensus: {s['median_shift']:.1f} bases"]
