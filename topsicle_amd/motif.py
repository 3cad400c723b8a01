"""Finding the telomere motif from the reads: `python -m topsicle_amd.motif`, and what `topsicle --pattern auto` runs first.

The reference needs --pattern and sends its user to other tools for it (README: Tandem Repeats Finder, tidk, or aligning reads to
chromosome ends).  Here every batch is resident in HBM anyway, so the question is put to the reads themselves: the census kernel
(HipScanner.motif_census; the rule is in include/topsicle_hip.h) answers, per read end, "which period between 4 and 32 repeats most
in the first 1000 bases, and what is the repeated word".  This module turns those per-end hits into a motif: ends whose support
reaches `min_support` vote for the canonical spelling of their unit, the motif with the most votes is the answer.

Both read ends are looked at "telomere first, C-strand 5'->3'" -- the orientation --pattern is given in (CCCTAA for human) -- so a
motif and its reverse complement are different rows of the table: which of the two the reads start with is the data's to say.
"""
from __future__ import annotations

import argparse
import csv
import os
import sys

import numpy as np

from . import batch, hiplib

LETTERS = "ACTG"                  # the packed batch's 2-bit codes
MIN_SUPPORT = 24                  # recurring 8-mers a read end needs to vote: synthetic telomeric ends (ONT and HiFi error rates, motifs of 6 to
                                  # 25 letters, 1000 bases) score >= 54, ends without a telomere <= 15
MIN_READ_ENDS = 5                 # votes the rank-1 motif needs before --pattern auto goes on with it
MOTIF_READS = 100000              # reads of the input looked at by default (0 = all of them)
CONTEXTS_PER_GPU = 2


def unit_string(code: int, period: int) -> str:
    """The letters of tps_motif_hit.unit: letter j in bits [2j, 2j+1], A C T G = 0 1 2 3."""
    code = int(code)
    return "".join(LETTERS[(code >> (2 * j)) & 3] for j in range(period))


def canonical(unit: str) -> str:
    """One spelling per repeat: a unit that is a power of a shorter word is reduced to that word (CCCTAACCCTAA -> CCCTAA), then the
    lexicographically smallest rotation is taken -- AACCCT for human, AAACCCT for A. thaliana, as the reference's README lists them.
    No reverse complement: the orientation is the data's."""
    n = len(unit)
    for d in range(1, n + 1):
        if n % d == 0 and unit[:d] * (n // d) == unit:
            unit = unit[:d]
            break
    return min(unit[i:] + unit[:i] for i in range(len(unit))) if unit else unit


def tally(hits, min_support: int = MIN_SUPPORT):
    """hits (MOTIF_HIT_DTYPE, any shape) -> rows (motif, period, read_ends, total_support), best first: by read ends that voted for
    the motif, then by their summed support, then by the string.  Only ends with support >= min_support (and > 0) vote."""
    h = np.asarray(hits).reshape(-1)
    h = h[(h["support"] >= max(int(min_support), 1)) & (h["period"] > 0)]
    votes: dict[str, list[int]] = {}
    spelled: dict[tuple[int, int], str] = {}
    for code, period, support in zip(h["unit"].tolist(), h["period"].tolist(), h["support"].tolist()):
        key = (code, period)
        if key not in spelled:
            spelled[key] = canonical(unit_string(code, period))
        v = votes.setdefault(spelled[key], [0, 0])
        v[0] += 1
        v[1] += support
    rows = [(m, len(m), v[0], v[1]) for m, v in votes.items()]
    rows.sort(key=lambda r: (-r[2], -r[3], r[0]))
    return rows


def input_files(paths):
    """The files main.analysis_run would process for each of `paths` (a file, or every file under a directory)."""
    out = []
    for p in [paths] if isinstance(paths, (str, os.PathLike)) else list(paths):
        if os.path.isdir(p):
            for root, _dirs, files in os.walk(p):
                out += [os.path.join(root, f) for f in files]
        else:
            out.append(p)
    return out


def open_engines(gpus: int = 1, device: int = 0):
    return [hiplib.HipScanner(device + i // CONTEXTS_PER_GPU) for i in range(max(1, gpus) * CONTEXTS_PER_GPU)]


def census_files(paths, engines, u_min=4, u_max=32, lo=0, hi=1000, min_len=0, max_reads=MOTIF_READS):
    """Every read-end hit of the first `max_reads` reads (0 = all) of the input, in file order: MOTIF_HIT_DTYPE[n, 2].  The files go
    through batch.EnginePool like a scan does -- the native readers (FASTA, FASTQ, gz, BGZF, BAM), the pinned staging buffers, one
    worker per context -- with a census of each resident batch in place of the scan."""
    job = batch.CensusJob(u_min, u_max, lo, hi, min_len)
    parts, seen = [], 0
    for path in input_files(paths):
        if max_reads and seen >= max_reads:
            break
        pool = batch.EnginePool(engines, two_pass="off")
        it = pool.scan_file_jobs(path, [job])
        try:
            for _pb, outs in it:
                hits = outs[0][0]
                if max_reads and seen + len(hits) > max_reads:
                    hits = hits[:max_reads - seen]
                parts.append(hits)
                seen += len(hits)
                if max_reads and seen >= max_reads:
                    break
        finally:
            it.close()                     # (stops the reader and the workers of a file left early)
    return np.concatenate(parts) if parts else np.zeros((0, 2), hiplib.MOTIF_HIT_DTYPE)


def find_motif(paths, engines=None, u_min=4, u_max=32, lo=0, hi=1000, min_support=MIN_SUPPORT, min_len=0, max_reads=MOTIF_READS,
               gpus=1, device=0):
    """(rows, n_reads): tally() of the census of the input's read ends, and how many reads were looked at.  `engines`: the contexts
    to use (main.analysis_run and the tests pass theirs); by default two per GPU are opened and closed here."""
    own = engines is None
    if own:
        engines = open_engines(gpus, device)
    try:
        hits = census_files(paths, engines, u_min, u_max, lo, hi, min_len, max_reads)
    finally:
        if own:
            for e in engines:
                e.close()
    return tally(hits, min_support), len(hits)


def format_table(rows, top: int = 10):
    """The table as lines of text: rank, motif, period, read ends, their share of all votes, total support."""
    total = sum(r[2] for r in rows)
    lines = ["rank  motif" + " " * 29 + "period  read_ends  share  total_support"]
    for i, (m, period, ends, support) in enumerate(rows[:top] if top else rows):
        lines.append(f"{i + 1:<4}  {m:<32}  {period:>6}  {ends:>9}  {ends / total:>5.3f}  {support:>13}")
    return lines


def write_csv(path, rows):
    total = sum(r[2] for r in rows)
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["rank", "motif", "period", "read_ends", "share", "total_support"])
        for i, (m, period, ends, support) in enumerate(rows):
            w.writerow([i + 1, m, period, ends, "%.4f" % (ends / total), support])


def verdict(rows, min_read_ends: int = MIN_READ_ENDS):
    """None if the rank-1 motif can be used, else the one-line reason why not."""
    if not rows:
        return "no read end reaches the minimum support: no repeat of the searched periods at the read ends"
    if rows[0][2] < min_read_ends:
        return f"only {rows[0][2]} read end(s) vote for the leading motif {rows[0][0]}; at least {min_read_ends} are needed"
    return None


def build_parser():
    p = argparse.ArgumentParser(description="Topsicle (MI355X build) - find the telomere repeat motif from the ends of long reads",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--inputDir", "-i", type=str, metavar="FILE/FOLDER", required=True, help="input file or directory (FASTA, FASTQ, .gz, BGZF, BAM)")
    p.add_argument("--outputDir", "-o", type=str, metavar="FOLDER", required=True, help="where motif_census.csv is written")
    p.add_argument("--minperiod", metavar="INT", type=int, default=4, help="shortest motif looked for")
    p.add_argument("--maxperiod", metavar="INT", type=int, default=hiplib.MOTIF_MAX_PERIOD, help="longest motif looked for (at most 32)")
    p.add_argument("--lo", metavar="INT", type=int, default=0, help="first base of a read end that is looked at")
    p.add_argument("--hi", metavar="INT", type=int, default=1000, help="end of the range of a read end that is looked at (at most 4096 bases)")
    p.add_argument("--minsupport", metavar="INT", type=int, default=MIN_SUPPORT, help="recurring 8-mers a read end needs to vote")
    p.add_argument("--minSeqLength", metavar="INT", type=int, default=9000, help="minimum length of a read that is looked at")
    p.add_argument("--motifreads", metavar="INT", type=int, default=MOTIF_READS, help="reads of the input that are looked at (0 = all)")
    p.add_argument("--top", metavar="INT", type=int, default=10, help="rows of the table that are printed (the CSV holds all)")
    p.add_argument("--gpus", metavar="INT", type=int, default=1, help="GPUs of this node to shard reads over")
    p.add_argument("--device", metavar="INT", type=int, default=0, help="index of the first GPU to use")
    return p


def main(argv=None, engines=None):
    args = build_parser().parse_args(argv)
    os.makedirs(args.outputDir, exist_ok=True)
    rows, n_reads = find_motif(args.inputDir, engines, args.minperiod, args.maxperiod, args.lo, args.hi, args.minsupport, args.minSeqLength,
                               args.motifreads, args.gpus, args.device)
    out = os.path.join(args.outputDir, "motif_census.csv")
    write_csv(out, rows)
    print(f"motif census of {n_reads} reads (both ends, bases {args.lo}..{args.hi}, periods {args.minperiod}..{args.maxperiod}, support >= {args.minsupport}):")
    for line in format_table(rows, args.top):
        print(line)
    print(f"written: {out}")
    why = verdict(rows)
    if why:
        print(why)
        return 1
    print(f"--pattern {rows[0][0]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
