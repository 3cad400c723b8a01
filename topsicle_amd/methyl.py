"""Subtelomere CpG methylation per read from the BAM MM / ML tags (`--methyl`; seqio.bam_mods, tps_bam_mods_spans;
HipScanner.mod_profile, tps_batch_mod_profile).

Dorado's and PacBio's BAM files carry per-base 5mC calls in the MM / ML aux tags: MM lists, per modification, how many C's of the read
as sequenced to skip between calls, ML the probability of each call as a byte.  The native reader walks the aux block of the records
with a stored boundary -- nothing of the others is touched -- and the kernel turns the skip counts into positions of the resident
read (a rank / select over its C's), keeps the calls that sit on a CpG inside [boundary - methyltract bins, boundary + methylbins
bins) and bins them by their distance from the boundary.  This module holds what the host adds: the regions, the two byte
thresholds, the files and the summary for the log.

A call is `high` when its probability (ML + 0.5) / 256 is at least --methylhigh and `low` when it is at most --methyllow; what lies
between counts as called but neither.  meth_fraction of a read = high / (high + low) over the bins behind the boundary; where the tag
says that skipped C's are unmodified (`C+m.` or no flag: mode implicit) the CpGs without a call join the denominator.

Only BAM batches carry tags: the reads of any other input get `untagged` rows.  Left out: MM / ML in FASTQ headers, groups on base N,
strand - (duplex) and ChEBI-only codes (all `nogroup`), more than one code per run, --refine's boundary as origin.  The thresholds
and the defaults rest on synthetic reads; no real library has been looked at.
"""
from __future__ import annotations

import math

import numpy as np

from . import analyses
from .analyses import median_cell

DEFAULT_BIN, DEFAULT_BINS, DEFAULT_TRACT, DEFAULT_HIGH, DEFAULT_LOW, DEFAULT_CODE = 500, 8, 2, 0.8, 0.2, "m"
BIN_RANGE, MAX_BINS, MAX_REGION = (16, 4096), 64, 16384
STATUS = ("ok", "none", "nogroup", "malformed", "clipped", "untagged")       # seqio.MODS_STATUS
OK, UNTAGGED = 0, 5


def thresholds(high: float, low: float):
    """(hi, lo) as bytes: the smallest ML whose probability (ML + 0.5) / 256 is >= high, the largest whose is <= low."""
    return math.ceil(256 * high - 0.5), math.floor(256 * low - 0.5)


class MethylSpec(analyses.BoundaryAnalysis):
    """What batch.Job(methyl=...) carries.  It needs the batch's records (needs_records): regions() reads the tags of the reads with a
    stored boundary out of them, and only the reads whose tags are `ok` get a region."""

    needs_records = True

    def __init__(self, bin_w: int = DEFAULT_BIN, bins: int = DEFAULT_BINS, tract: int = DEFAULT_TRACT, high: float = DEFAULT_HIGH, low: float = DEFAULT_LOW,
                 code: str = DEFAULT_CODE, sink=None):
        self.w, self.nb0, self.nb1, self.code, self.sink = int(bin_w), int(tract), int(bins), code, sink
        self.hi, self.lo = thresholds(high, low)

    def regions(self, res, prm, recs):
        from . import seqio, variants
        _b, boundary = variants.tract_bounds(res, *self.scan_geometry(prm))
        mods = seqio.bam_mods(recs, boundary > 0, self.code)
        ok = (boundary > 0) & (mods.status == OK)
        origin = np.where(ok, boundary, 0).astype(np.int32)
        begin = np.where(ok, np.maximum(0, origin.astype(np.int64) - self.nb0 * self.w), 0).astype(np.int32)
        end = np.where(ok, origin.astype(np.int64) + self.nb1 * self.w, 0).astype(np.int32)
        return begin, end, origin, mods

    def empty(self, n):
        """what reads without a region get; a batch that is not resident at all came in heads mode: no BAM, no tags"""
        from . import hiplib
        return (np.zeros(n, hiplib.MOD_ROW_DTYPE), np.zeros((n, self.nb0 + self.nb1), hiplib.MOD_BIN_DTYPE), np.full(n, UNTAGGED, np.int32),
                np.zeros(n, np.uint8))

    def launch(self, eng, slot, tails, begin, end, origin, mods):
        if not (end > begin).any():                # (no tagged read with a boundary: nothing to launch)
            rows, bins = self.empty(len(tails))[:2]
        else:
            rows, bins = eng.mod_profile(slot, tails, begin, end, origin, mods.mod_off, mods.delta, mods.prob, w=self.w, nb0=self.nb0, nb1=self.nb1,
                                         hi=self.hi, lo=self.lo)
        return rows, bins, mods.status.copy(), mods.mode.copy()


def check(bin_w: int, bins: int, tract: int, high: float, low: float, code: str):
    """None, or what `--methyl` needs, in words: before any input file is read."""
    if not (BIN_RANGE[0] <= bin_w <= BIN_RANGE[1]):
        return f"--methylbin in {BIN_RANGE[0]}..{BIN_RANGE[1]}"
    if bins < 1 or tract < 0 or bins + tract > MAX_BINS:
        return f"--methylbins of at least 1, --methyltract of at least 0 and at most {MAX_BINS} bins together"
    if (bins + tract) * bin_w > MAX_REGION:
        return f"a region of at most {MAX_REGION} bases: (--methylbins + --methyltract) x --methylbin is {(bins + tract) * bin_w}"
    if not (0.0 <= low < high <= 1.0):
        return "0 <= --methyllow < --methylhigh <= 1"
    hi, lo = thresholds(high, low)
    if not (0 <= lo < hi <= 255):
        return f"--methylhigh and --methyllow that a byte can meet: they come out as ML >= {hi} and ML <= {lo}"
    if len(code) != 1 or not ("a" <= code <= "z"):
        return "--methylcode of one lower-case letter (m: 5mC, h: 5hmC)"
    return None


class Collector(analyses.Collector):
    """The sink of one k of a run.  A row: (file, readID, tail, telo_length, the read's row, its bins, status, mode)."""

    def __init__(self, bin_w: int = DEFAULT_BIN, bins: int = DEFAULT_BINS, tract: int = DEFAULT_TRACT, high: float = DEFAULT_HIGH, low: float = DEFAULT_LOW,
                 code: str = DEFAULT_CODE):
        super().__init__()
        self.high, self.low = float(high), float(low)
        self.spec = MethylSpec(bin_w, bins, tract, high, low, code, self)

    def keep_row(self, out, i, file, rid, tail, telo, length):
        rows, bins, status, mode = out
        return file, rid, tail, telo, rows[i].copy(), bins[i].copy(), int(status[i]), int(mode[i])

    def read_row(self, file, rid, tail, telo, row, bins, status, mode):
        """One line of methyl_{k}.csv, and (status, meth_fraction or None)."""
        from . import hiplib
        if status == OK and int(row["flags"]) & hiplib.MOD_BAD:
            status = STATUS.index("malformed")     # an entry beyond the read's last C: the tag does not belong to these bases
        head = [file, rid, "forward" if tail == 0 else "reverse", telo, STATUS[status]]
        if status != OK:
            return head + [""] * 10, status, None
        behind = bins[self.spec.nb0:]
        cpg, called, high, low, total = (int(behind[f].sum(dtype=np.int64)) for f in ("cpg", "called", "high", "low", "sum"))
        frac = fraction(cpg, called, high, low, mode)
        return head + ["explicit" if mode else "implicit", int(row["c_total"]), int(row["entries"]), int(row["off_context"]), cpg, called, high, low,
                       "" if frac is None else "%.4f" % frac, "" if called == 0 else "%.4f" % ((total / called + 0.5) / 256)], status, frac

    def finish(self, paths):
        """(read rows, profile rows, per-read (status, fraction), stats) of the run."""
        kept = self.rows_in_order(paths)
        done = [self.read_row(*r) for r in kept]
        read_rows = [d[0] for d in done]
        nb0, nb, w = self.spec.nb0, self.spec.nb0 + self.spec.nb1, self.spec.w
        tot = {f: np.zeros(nb, np.int64) for f in ("cpg", "called", "high", "low", "sum")}
        reads = np.zeros(nb, np.int64)
        for r, d in zip(kept, done):
            if d[1] == OK:
                for f in tot:
                    tot[f] += r[5][f]
                reads += r[5]["cpg"] > 0
        profile_rows = []
        for b in range(nb):
            hl = int(tot["high"][b] + tot["low"][b])
            profile_rows.append([b - nb0, (b - nb0) * w, (b - nb0 + 1) * w, int(reads[b])] + [int(tot[f][b]) for f in ("cpg", "called", "high", "low")] +
                                ["" if hl == 0 else "%.4f" % (int(tot["high"][b]) / hl),
                                 "" if tot["called"][b] == 0 else "%.4f" % ((int(tot["sum"][b]) / int(tot["called"][b]) + 0.5) / 256)])
        fracs = [d[2] for d in done if d[2] is not None]
        stats = {"reads": len(done), "counts": {s: sum(1 for d in done if d[1] == i) for i, s in enumerate(STATUS)}, "with_fraction": len(fracs),
                 "fraction_median": median_cell(fracs)}
        return read_rows, profile_rows, [(d[1], d[2]) for d in done], stats


def fraction(cpg: int, called: int, high: int, low: int, mode: int):
    """high / (high + low), the CpGs without a call in the denominator where skipped C's are unmodified (mode 0); None: nothing to divide by"""
    den = high + low + (0 if mode else max(0, cpg - called))
    return None if den == 0 else high / den


READ_HEADER = ["file", "readID", "tail", "telo_length", "tags", "mode", "c_total", "entries", "off_context", "cpg", "called", "high", "low", "meth_fraction",
               "mean_prob"]
PROFILE_HEADER = ["bin", "from", "to", "reads", "cpg", "called", "high", "low", "meth_fraction", "mean_prob"]
ENDS_HEADER = ["end", "reads", "tagged", "cpg", "called", "meth_fraction_median", "telo_median"]


def end_rows(read_rows, per_read, end_read_rows):
    """One row per end group: end_reads_{k}.csv and methyl_{k}.csv hold the same reads in the same order."""
    assert len(read_rows) == len(end_read_rows) and all(a[1] == b[1] for a, b in zip(read_rows, end_read_rows))
    groups = sorted({int(r[7]) for r in end_read_rows} - {0})
    out = []
    for g in groups:
        mem = [i for i, r in enumerate(end_read_rows) if int(r[7]) == g]
        tagged = [i for i in mem if per_read[i][0] == OK]
        out.append([g, len(mem), len(tagged), sum(read_rows[i][9] for i in tagged), sum(read_rows[i][10] for i in tagged),
                    median_cell([per_read[i][1] for i in tagged if per_read[i][1] is not None]), median_cell([read_rows[i][3] for i in tagged])])
    return out


def summary(col: Collector, stats) -> list[str]:
    """Log lines for a run's methylation rows."""
    s = col.spec
    counts = ", ".join(f"{name} {stats['counts'][name]}" for name in STATUS)
    med = stats["fraction_median"]
    return [f"methylation: {stats['reads']} reads with a boundary, code {s.code}, {s.nb0} + {s.nb1} bins of {s.w} bases around it "
            f"(high: ML >= {s.hi}, low: ML <= {s.lo})",
            f"  tags: {counts}",
            f"  median meth_fraction of {stats['with_fraction']} reads: {med if med != '' else 'n/a'}"]


# ---- the CLI's side (main.ANALYSES)
FLAG = "methyl"
POWER_NOTE = None


def cli_check(args, root: str):
    from . import seqio
    why = check(args.methylbin, args.methylbins, args.methyltract, args.methylhigh, args.methyllow, args.methylcode)
    if why is None and not any(seqio.is_bam(f) for f in input_files(args.inputDir)):
        why = "BAM input: the MM / ML tags are read from BAM records, and no input file is one"
    return why


def input_files(input_dir):
    """The run's input files, as main.analysis_run lists them."""
    import os
    if os.path.isdir(input_dir):
        return [os.path.join(root, f) for root, _dirs, files in os.walk(input_dir) for f in files]
    return [input_dir] if os.path.exists(input_dir) else []


def cli_collector(args, unit: str, slide: int):
    return Collector(args.methylbin, args.methylbins, args.methyltract, args.methylhigh, args.methyllow, args.methylcode)


def finish_and_write(args, k, col, filenames, engines):
    """Writes methyl_{k}.csv and methyl_profile_{k}.csv, and methyl_ends_{k}.csv where --ends has grouped the same reads; yields the
    log lines."""
    read_rows, profile_rows, per_read, stats = col.finish(filenames)
    tables = [("methyl", READ_HEADER, read_rows), ("methyl_profile", PROFILE_HEADER, profile_rows)]
    ends_col = next((mine.get("ends") for mine in getattr(args, "analysis_collectors", []) if mine.get(FLAG) is col), None)
    if ends_col is not None and getattr(ends_col, "read_rows", None) is not None:
        tables.append(("methyl_ends", ENDS_HEADER, end_rows(read_rows, per_read, ends_col.read_rows)))
    yield analyses.write_tables(args.outputDir, k, "methylation", tables)
    yield from summary(col, stats)
