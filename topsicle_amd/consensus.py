"""A consensus subtelomere per end group (`--ends --anchor --consensus`; HipScanner.align_windows).

`--anchor` places every grouped read on its group's reference read -- a raw read, with a raw read's errors.  Here every anchored
member of a group is aligned base by base against that reference window inside a band of 64 diagonals centred on the anchor's offset
(tps_window_align, one wave per pair), the columns' votes are piled per group on the GPU, and the host calls one letter per column
from them: a sequence of the group's own that has a small fraction of a read's errors.  A second call aligns every member against its
group's consensus; its distance is the quality figure a user can read where no truth exists.  Written as FASTA behind error-free
repeats of the motif, the consensus is a reference `--endref` takes in the next run: end groups of two runs become comparable.

This module holds what the host adds: the rows of the two calls, the consensus rule, the four files and the summary for the log.
Only a report: no other output changes.  Left out: quality values, more than two inserted letters per site, a second polishing round,
splitting a group whose reads anchor at two places, affine gaps (DESIGN, section 8).
"""
from __future__ import annotations

import numpy as np

from . import anchor

DEFAULT_MIN_DEPTH = 3
MAX_SPAN = 4096
REFERENCE_TELO = 2500             # bases of the motif in front of a record of end_reference_{k}.fa, at the least
LETTERS = "ACTG"                  # code 0 1 2 3, as tps_batch_end_window packs them
NONE, EDGE, DELETED = 1, 2, 4     # tps_window_align: the two flags, the state of a deleted column

GROUP_HEADER = ["end", "reads", "anchored", "used", "edge", "reference", "first_column", "last_column", "length", "min_depth", "median_depth",
                "substituted", "deleted", "inserted", "median_dist_before", "median_dist_after"]
READ_HEADER = ["file", "readID", "end", "dist", "q_begin", "q_end", "r_begin", "r_end", "edge", "used", "dist_after"]

FLAG = "consensus"                # (main.EARLY_CHECKS; the rest of its CLI side is inside ends.finish_and_write)


def check(with_ends: bool, with_anchor: bool, min_depth: int = DEFAULT_MIN_DEPTH):
    """None, or what is wrong, in words for the command line."""
    if not with_ends or not with_anchor or min_depth < 1:
        return "--ends and --anchor (the anchored members of a group are what is aligned) and --consensusmindepth of at least 1"
    return None


def cli_check(args, root: str):
    return check(getattr(args, "ends", False), getattr(args, "anchor", False), args.consensusmindepth)


def letters_of(codes_row, length: int) -> np.ndarray:
    """The 2-bit codes of a window's letters, one per entry."""
    words = np.repeat(np.asarray(codes_row, np.uint32), 16)[:length]
    return ((words >> (2 * (np.arange(length, dtype=np.uint32) & 15))) & 3).astype(np.int64)


def pack(codes, span: int) -> np.ndarray:
    """A codes row of `span` letters from 2-bit codes."""
    row = np.zeros(((span + 15) // 16) * 16, np.uint32)
    row[:len(codes)] = codes
    return (row.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def call_consensus(pile, ref_letters, min_depth: int = DEFAULT_MIN_DEPTH):
    """The consensus of one pile row (int[span][13]: A C T G del, ins1[4], ins2[4]) over its reference window's letters (codes): None
    without a column of depth >= min_depth, else dict(codes, first, last, cpos, depth, substituted, deleted, inserted).
      * depth = the sum of the five states; the consensus runs from the first to the last column with depth >= min_depth;
      * a column inside with less takes the reference's letter;
      * else: ins1's most-voted letter first if 2 * sum(ins1) > depth (ties to the smallest code), then ins2's the same way if ins1
        was emitted; then the most-voted state, ties to the reference's own letter if it is among them, else to the smallest state;
        "deleted" emits nothing;
      * cpos[j] = the consensus position of column j's own letter (where it would stand, for a deleted one), continued at one
        letter per column in front of `first` and behind `last`."""
    m = len(ref_letters)
    pile = np.asarray(pile, np.int64)[:m]
    depth = pile[:, :5].sum(axis=1)
    deep = np.nonzero(depth >= min_depth)[0]
    if not len(deep):
        return None
    first, last = int(deep[0]), int(deep[-1])
    out, cpos = [], np.zeros(m, np.int64)
    substituted = deleted = inserted = 0
    for j in range(first, last + 1):
        own = int(ref_letters[j])
        pick = own
        if depth[j] >= min_depth:
            if 2 * pile[j, 5:9].sum() > depth[j]:
                out.append(int(np.argmax(pile[j, 5:9])))                       # (argmax: the first of equal maxima)
                inserted += 1
                if 2 * pile[j, 9:13].sum() > depth[j]:
                    out.append(int(np.argmax(pile[j, 9:13])))
                    inserted += 1
            states = pile[j, :5]
            pick = own if states[own] == states.max() else int(np.argmax(states))
        cpos[j] = len(out)
        if pick == DELETED:
            deleted += 1
        else:
            out.append(pick)
            substituted += pick != own
    cpos[:first] = cpos[first] + np.arange(-first, 0)
    cpos[last + 1:] = cpos[last] + np.arange(1, m - last)
    return dict(codes=np.array(out, np.int64), first=first, last=last, cpos=cpos, depth=depth[first:last + 1], substituted=int(substituted),
                deleted=deleted, inserted=inserted)


def column_at(cons, column: int) -> int:
    """The consensus position of a column of the reference window that may lie outside it."""
    cpos = cons["cpos"]
    if column < 0:
        return int(cpos[0]) + column
    if column >= len(cpos):
        return int(cpos[-1]) + column - (len(cpos) - 1)
    return int(cpos[column])


def reference_record(unit: str, cons_letters: str, boundary: int, min_seq_length: int):
    """(record, T): T bases of error-free repeats of the motif, then the consensus from its boundary column on (from 0 where that is
    negative).  T = the smallest multiple of the motif's length with T >= 2500 and T + the rest > min_seq_length: `--endref` scans
    the pieces with the run's own parameters, and its length filter keeps what is LONGER than --minSeqLength."""
    rest = cons_letters[max(boundary, 0):]
    need = max(REFERENCE_TELO, min_seq_length + 1 - len(rest))
    reps = -(-need // len(unit))
    return unit * reps + rest, reps * len(unit)


def _per_thousand(dist, columns):
    return 1000.0 * dist / np.maximum(columns, 1)


def run(rows, read_rows, a_reads, a_groups, engine, unit: str, span: int, min_depth: int = DEFAULT_MIN_DEPTH, min_seq_length: int = 0):
    """The consensus of every group of a run.  `rows`, `read_rows`: as anchor.run takes them; `a_reads`, `a_groups`: the rows of
    anchored_reads_{k}.csv and anchored_ends_{k}.csv it returned; `engine`: anything with align_windows.  Returns (records of
    end_consensus_{k}.fa as (header, letters), rows of end_consensus_{k}.csv, rows of consensus_reads_{k}.csv, records of
    end_reference_{k}.fa, stats for the log)."""
    n = len(rows)
    end = np.array([r[7] for r in read_rows], np.int64).reshape(n)
    links = np.array([r[8] for r in read_rows], np.int64).reshape(n)
    begin = np.array([r[4] for r in rows], np.int64).reshape(n)
    ref = anchor.references(end, links)
    anchored = np.array([r[10] != "" for r in a_reads], bool).reshape(n)
    offset = np.array([r[6] if r[10] != "" else 0 for r in a_reads], np.int64).reshape(n)
    boundary_of = {int(r[0]): int(r[4]) for r in a_groups if r[4] != ""}
    members = np.nonzero(anchored)[0]
    groups = [int(g) for g in np.unique(end[members])]
    g_row = {g: p for p, g in enumerate(groups)}
    stat1 = np.zeros((n, 6), np.int32)
    stat2 = np.zeros((n, 6), np.int32)
    cons = {}
    cut = []
    if len(members):
        ref_read = {g: int(ref[members[end[members] == g][0]]) for g in groups}
        codes = np.stack([rows[i][9] for i in members]).astype(np.uint32)
        length = np.array([rows[i][8] for i in members], np.int32)
        ref_codes = np.stack([rows[ref_read[g]][9] for g in groups]).astype(np.uint32)
        ref_length = np.array([rows[ref_read[g]][8] for g in groups], np.int32)
        row_of = np.array([g_row[int(end[i])] for i in members], np.int32)
        # first pass: every anchored member against its group's reference window on the anchor's diagonal, one pile row per group
        st, _cols, pile = engine.align_windows(codes, length, ref_codes, ref_length, row_of, offset[members].astype(np.int32), span, cols=False,
                                               pile_row=row_of, n_pile=len(groups))
        stat1[members] = st
        for g in groups:
            c = call_consensus(pile[g_row[g]], letters_of(ref_codes[g_row[g]], int(ref_length[g_row[g]])), min_depth)
            if c is not None:
                if len(c["codes"]) > MAX_SPAN:
                    cut.append(g)
                    c["codes"] = c["codes"][:MAX_SPAN]
                cons[g] = c
        # second pass: every anchored member of a group with a consensus against it; the band sits where the first path's middle went
        again = np.array([p for p, i in enumerate(members) if int(end[i]) in cons], np.int64)
        if len(again):
            have = [g for g in groups if g in cons]
            c_row = {g: p for p, g in enumerate(have)}
            span2 = max(span, max(len(cons[g]["codes"]) for g in have))
            cdw2 = (span2 + 15) // 16
            q2 = np.zeros((len(again), cdw2), np.uint32)
            q2[:, :codes.shape[1]] = codes[again]
            r2 = np.stack([pack(cons[g]["codes"], span2) for g in have])
            r2_length = np.array([len(cons[g]["codes"]) for g in have], np.int32)
            centre2 = np.zeros(len(again), np.int32)
            for p, m in enumerate(again):
                i = members[m]
                c = cons[int(end[i])]
                jm = (int(st[m, 3]) + int(st[m, 4])) // 2
                jm = min(max(jm, 0), len(c["cpos"]) - 1) if len(c["cpos"]) else 0
                centre2[p] = np.clip(offset[i] + (c["cpos"][jm] - jm if len(c["cpos"]) else 0), -MAX_SPAN, MAX_SPAN)
            ref2 = np.array([c_row[int(end[members[m]])] for m in again], np.int32)
            stat2[members[again]] = engine.align_windows(q2, length[again], r2, r2_length, ref2, centre2, span2, cols=False)[0]
    aligned1 = anchored & ((stat1[:, 5] & NONE) == 0)
    used = aligned1 & (stat1[:, 5] == 0)
    edge = aligned1 & ((stat1[:, 5] & EDGE) != 0)
    has_after = np.array([anchored[i] and int(end[i]) in cons and (stat2[i, 5] & NONE) == 0 for i in range(n)], bool)
    before = _per_thousand(stat1[:, 0].astype(np.float64), stat1[:, 4] - stat1[:, 3])
    after = _per_thousand(stat2[:, 0].astype(np.float64), stat2[:, 4] - stat2[:, 3])
    out_reads = []
    for i, r in enumerate(rows):
        row = [r[0], r[1], int(end[i])]
        if aligned1[i]:
            row += [int(x) for x in stat1[i, :5]] + [int(edge[i]), int(used[i]), int(stat2[i, 0]) if has_after[i] else ""]
        else:
            row += [""] * 8
        out_reads.append(row)
    records, references, out_groups = [], [], []
    too_long = 0
    for g in range(1, int(end.max()) + 1 if n else 1):
        mem = np.nonzero(end == g)[0]
        ref_id = rows[ref[mem[0]]][1]
        row = [g, len(mem), int(anchored[mem].sum()), int(used[mem].sum()), int(edge[mem].sum()), ref_id]
        c = cons.get(g)
        if c is None:
            out_groups.append(row + [""] * 10)
            continue
        letters = "".join(LETTERS[x] for x in c["codes"])
        b = [float(before[i]) for i in mem if used[i]]
        a = [float(after[i]) for i in mem if used[i] and has_after[i]]
        row += [c["first"], c["last"], len(letters), int(c["depth"].min()), "%.1f" % np.median(c["depth"]), c["substituted"], c["deleted"], c["inserted"],
                "%.1f" % np.median(b) if b else "", "%.1f" % np.median(a) if a else ""]
        out_groups.append(row)
        boundary = column_at(c, boundary_of[g] - int(begin[ref[mem[0]]]))
        records.append((f"end{g} reads={len(mem)} used={int(used[mem].sum())} reference={ref_id} boundary={boundary}", letters))
        record, telo = reference_record(unit, letters, boundary, min_seq_length)
        references.append((f"end{g} consensus of {int(used[mem].sum())} reads behind {telo} bases of {unit}", record))
        too_long = max(too_long, telo)
    n_used = int(used.sum())
    stats = dict(groups=len(out_groups), with_consensus=len(records), anchored=int(anchored.sum()), grouped=int((end > 0).sum()), used=n_used, edge=int(edge.sum()),
                 median_before=float(np.median(before[used])) if n_used else 0.0,
                 median_after=float(np.median(after[used & has_after])) if (used & has_after).any() else 0.0, cut=cut, telo=too_long)
    return records, out_groups, out_reads, references, stats


def write_fasta(path: str, records, width: int = 80):
    with open(path, "w") as fh:
        for header, letters in records:
            fh.write(f">{header}\n")
            fh.write("".join(letters[i:i + width] + "\n" for i in range(0, len(letters), width)))


def summary(stats, min_depth: int, maxlengthtelo: int) -> list[str]:
    """The log lines of one k."""
    s = stats
    lines = [f"end consensus: {s['with_consensus']} of {s['groups']} end groups have a consensus (columns of depth {min_depth} or more)",
             f"  {s['used']} of {s['anchored']} anchored reads used, {s['edge']} touched the band's edge, {s['grouped'] - s['anchored']} grouped reads not anchored",
             f"  median edits per 1000 aligned columns: {s['median_before']:.1f} against the reference read, {s['median_after']:.1f} against the consensus"]
    for g in s["cut"]:
        lines.append(f"  the consensus of end {g} was cut at {MAX_SPAN} letters for the second pass")
    if s["telo"] > maxlengthtelo:
        lines.append(f"  end_reference holds {s['telo']} bases of the motif, more than --maxlengthtelo {maxlengthtelo}: the file will not serve --endref at these settings")
    return lines
