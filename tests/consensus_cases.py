"""Test helper: what `--ends --anchor --consensus` has to write for a planted-end set of tests/ends_cases.py, and what `--endref` on the
reference it wrote has to say -- shared by tests/test_consensus_cli.py (host emulation) and tests/test_gpu_consensus.py (GPU)."""
import csv
import os

import numpy as np

import align_oracle as orc
import ends_cases as ec
import place_cases as pc
from topsicle_amd import consensus

NEW = ("end_consensus_{k}.fa", "end_consensus_{k}.csv", "consensus_reads_{k}.csv", "end_reference_{k}.fa")
MIN_SEQ = 5000                    # --minSeqLength of the runs: the 6 000-base reads pass
BARS = {"ONT": 16, "HIFI": 2}     # edits of a consensus without its first 400 letters inside the planted subtelomere


def _rows(path):
    return list(csv.reader(open(path)))


def fasta(path):
    out, name = [], None
    for line in open(path):
        if line.startswith(">"):
            name = line[1:].strip()
            out.append([name, ""])
        else:
            out[-1][1] += line.strip()
    return out


def check_cli_outputs(outdir, ident, k=4, min_depth=consensus.DEFAULT_MIN_DEPTH):
    """The four files are consistent with each other, with anchored_reads_{k}.csv and with end_reads_{k}.csv; every planted end has a
    consensus within its bar.  Returns the groups' edits."""
    motif, err = ident.rsplit("_", 1)
    truth = ec.detection_reads(ident)[1]
    subs = pc.detection_subs(ident)
    e_rows = _rows(os.path.join(outdir, f"end_reads_{k}.csv"))[1:]
    a_rows = _rows(os.path.join(outdir, f"anchored_reads_{k}.csv"))[1:]
    a_groups = {r[0]: r for r in _rows(os.path.join(outdir, f"anchored_ends_{k}.csv"))[1:]}
    c_reads = _rows(os.path.join(outdir, f"consensus_reads_{k}.csv"))
    assert c_reads[0] == consensus.READ_HEADER == ["file", "readID", "end", "dist", "q_begin", "q_end", "r_begin", "r_end", "edge", "used", "dist_after"]
    c_reads = c_reads[1:]
    assert [r[:3] for r in c_reads] == [[e[0], e[1], e[7]] for e in e_rows]                  # one row per row of end_reads, in its order
    for c, a in zip(c_reads, a_rows):
        if a[10] == "":                            # not anchored: not aligned
            assert c[3:] == [""] * 8
            continue
        assert all(x != "" for x in c[3:10]) and c[9] == str(int(c[8] == "0")) and 0 <= int(c[4]) <= int(c[5]) and 0 <= int(c[6]) <= int(c[7]) <= ec.SPAN
    c_groups = _rows(os.path.join(outdir, f"end_consensus_{k}.csv"))
    assert c_groups[0] == consensus.GROUP_HEADER == ["end", "reads", "anchored", "used", "edge", "reference", "first_column", "last_column", "length", "min_depth",
                                                     "median_depth", "substituted", "deleted", "inserted", "median_dist_before", "median_dist_after"]
    c_groups = c_groups[1:]
    assert [r[0] for r in c_groups] == sorted(a_groups, key=int)
    records = fasta(os.path.join(outdir, f"end_consensus_{k}.fa"))
    references = fasta(os.path.join(outdir, f"end_reference_{k}.fa"))
    with_consensus = [r for r in c_groups if r[8] != ""]
    assert [h.split()[0] for h, _ in records] == [h.split()[0] for h, _ in references] == [f"end{r[0]}" for r in with_consensus]
    edits = []
    for row, (header, letters), (_rh, record) in zip(with_consensus, records, references):
        mem = [(c, a) for c, a in zip(c_reads, a_rows) if c[2] == row[0]]
        used = [c for c, _a in mem if c[9] == "1"]
        assert (int(row[1]), int(row[2]), int(row[3]), int(row[4])) == (len(mem), sum(a[10] != "" for _c, a in mem), len(used), sum(c[8] == "1" for c, _a in mem))
        assert row[5] == a_groups[row[0]][3] and int(row[8]) == len(letters) and int(row[9]) >= 0 and int(row[6]) <= int(row[7])
        assert len(letters) == int(row[7]) - int(row[6]) + 1 - int(row[12]) + int(row[13])  # the reference's columns, less the deleted, plus the inserted
        before = np.median([1000.0 * int(c[3]) / max(int(c[7]) - int(c[6]), 1) for c in used])
        assert row[14] == "%.1f" % before and float(row[15]) <= float(row[14])
        f = dict(x.split("=") for x in header.split()[1:])
        assert (f["reads"], f["used"], f["reference"]) == (row[1], row[3], row[5])
        rest = letters[max(int(f["boundary"]), 0):]
        telo = len(record) - len(rest)
        assert record == motif * (telo // len(motif)) + rest and telo % len(motif) == 0 and telo >= consensus.REFERENCE_TELO
        # the smallest such T: the scan's length filter keeps a record LONGER than --minSeqLength
        assert len(record) > MIN_SEQ and (telo - len(motif) < consensus.REFERENCE_TELO or len(record) - len(motif) <= MIN_SEQ)
        planted = {truth[int(c[1][4:])] for c, _a in mem}
        assert len(planted) == 1 and 0 not in planted
        edits.append(orc.infix_distance(letters[400:], subs[planted.pop() - 1]))
    assert len(edits) == ec.N_ENDS and max(edits) <= BARS[err], edits
    return edits


def check_named_by_own_reference(outdir, k=4):
    """`--endref end_reference_{k}.fa` of the same reads: every group is named to its own end{g} record with agree = named; no
    unrelated read is named."""
    refs = _rows(os.path.join(outdir, f"ref_ends_{k}.csv"))[1:]
    heads = [r for r in refs if r[2] == "head"]
    assert [r[0] for r in heads] == [f"end{g}_head" for g in range(1, ec.N_ENDS + 1)] and all(r[9] == "1" for r in heads), refs
    assert all(r[9] == "0" for r in refs if r[2] == "tail")
    groups = _rows(os.path.join(outdir, f"named_ends_{k}.csv"))[1:]
    assert len(groups) == ec.N_ENDS
    for r in groups:
        assert r[3] == f"end{r[0]}_head" and r[4] == r[2] and int(r[2]) >= 10 and r[5] == "0", r
    e_rows = _rows(os.path.join(outdir, f"end_reads_{k}.csv"))[1:]
    named = _rows(os.path.join(outdir, f"named_reads_{k}.csv"))[1:]
    for r, e in zip(named, e_rows):
        if e[7] == "0":
            assert r[5] == "", r
        elif r[5] != "":
            assert r[5] == f"end{e[7]}_head", r
