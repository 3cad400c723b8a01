"""The consensus subtelomere of an end group (topsicle_amd/consensus.py) on the six planted-end sets of tests/ends_cases.py: groups and
references by the host rule (anchor_cases.detection_rows), offsets by the anchoring oracle (anchor_oracle.window_offsets), the two
passes by the alignment oracle (tests/align_oracle.py) -- and the same through consensus.run on the host emulation of the kernel,
which has to give the oracle's letters.

What the oracle gives (6 ends x 12 reads per set, windows at the planted boundary +- 300, min depth 3; the consensus and every member
window without their first 400 letters, scored by infix edit distance in the planted subtelomere; per set the six groups' min - max):

    set                              consensus    best single member    edits / 1000 columns before -> after (medians' range)
    CCCTAA_ONT                         1 - 9          70 - 80             105.2 - 121.5  ->  59.9 - 63.3
    AAACCCT_ONT                        0 - 6          72 - 88             105.9 - 115.4  ->  57.9 - 61.2
    ACGGATGTCTAACTTCTTGGTGT_ONT        0 - 9          71 - 85             100.8 - 119.9  ->  56.3 - 65.1
    the three HiFi sets                0 in all 18 groups

(Before: a read against another read, two reads' errors; after: a read against the consensus, its own errors alone.)
No anchored pair of the 432 touches the band's edge.
"""
import functools

import numpy as np
import pytest

import align_oracle as orc
import anchor_cases as ac
import anchor_oracle as ao
import ends_cases as ec
import place_cases as pc
from topsicle_amd import anchor, consensus

MIN_DEPTH, SKIP = 3, 400


@functools.lru_cache(maxsize=None)
def planted(ident):
    """Both passes of a planted set on the oracle: dict(members, group of each, refs, offset, stat1, cons per group, stat2, truth of
    each group)."""
    rows = ac.detection_rows(ident)
    g_end, _links = ac.detection_groups(ident)
    truth = ec.detection_reads(ident)[1]
    offset, votes, second = ao.window_offsets(rows["windows"], rows["keeps"], rows["ref"], ec.K)
    members = [i for i in range(len(g_end)) if g_end[i] and votes[i] >= ac.MIN_VOTES and votes[i] >= ac.RATIO * second[i]]
    groups = sorted({g_end[i] for i in members})
    ref_read = {g: rows["ref"][[i for i in members if g_end[i] == g][0]] for g in groups}
    refs = [rows["windows"][ref_read[g]] for g in groups]
    row_of = [groups.index(g_end[i]) for i in members]
    queries = [rows["windows"][i] for i in members]
    centre = [int(offset[i]) for i in members]
    stat1, _cols, pile = orc.window_align(queries, refs, row_of, centre, ec.SPAN, row_of, len(groups))
    cons = [orc.consensus(pile[p], refs[p], MIN_DEPTH) for p in range(len(groups))]
    assert all(c is not None for c in cons)
    centre2 = []
    for m, p in enumerate(row_of):
        jm = (int(stat1[m, 3]) + int(stat1[m, 4])) // 2
        centre2.append(centre[m] + cons[p][3][jm] - jm)
    stat2, _, _ = orc.window_align(queries, [c[0] for c in cons], row_of, centre2, max(ec.SPAN, max(len(c[0]) for c in cons)))
    return dict(members=members, row_of=row_of, groups=groups, refs=refs, queries=queries, centre=centre, stat1=stat1, pile=pile, cons=cons, stat2=stat2,
                truth=[truth[ref_read[g]] for g in groups], ref_read=ref_read)


@pytest.mark.parametrize("ident", ec.DETECT_IDS)
def test_no_anchored_pair_touches_the_bands_edge(ident):
    """A condition, not a measurement: 64 diagonals centred on the anchor's offset hold every path of the planted sets."""
    p = planted(ident)
    assert len(p["members"]) == ec.N_ENDS * ec.PER_END and (p["stat1"][:, 5] == 0).all() and (p["stat2"][:, 5] == 0).all()


@pytest.mark.parametrize("ident", ec.DETECT_IDS)
def test_consensus_is_close_to_the_planted_subtelomere(ident):
    """ONT: at most 16 edits per group and at most a quarter of the best member's figure scored the same way; HiFi: at most 2."""
    p = planted(ident)
    subs = pc.detection_subs(ident)
    ont = ident.endswith("_ONT")
    figures = []
    for g, c in enumerate(p["cons"]):
        sub = subs[p["truth"][g] - 1]
        edits = orc.infix_distance(c[0][SKIP:], sub)
        best = min(orc.infix_distance(q[SKIP:], sub) for q, r in zip(p["queries"], p["row_of"]) if r == g) if ont else None
        figures.append((edits, best))
    print(f"{ident}: consensus edits {min(e for e, _ in figures)} - {max(e for e, _ in figures)}" +
          (f", best single member {min(b for _, b in figures)} - {max(b for _, b in figures)}" if ont else ""))
    for edits, best in figures:
        if ont:
            assert edits <= 16 and 4 * edits <= best, figures
        else:
            assert edits <= 2, figures


@pytest.mark.parametrize("ident", [i for i in ec.DETECT_IDS if i.endswith("_ONT")])
def test_second_pass_is_closer_than_the_first(ident):
    """median_dist_after < median_dist_before in every ONT group (edits per 1 000 aligned reference columns)."""
    p = planted(ident)
    before = 1000.0 * p["stat1"][:, 0] / (p["stat1"][:, 4] - p["stat1"][:, 3])
    after = 1000.0 * p["stat2"][:, 0] / (p["stat2"][:, 4] - p["stat2"][:, 3])
    rows = np.array(p["row_of"])
    meds = [(float(np.median(before[rows == g])), float(np.median(after[rows == g]))) for g in range(len(p["groups"]))]
    print(f"{ident}: median edits per 1000 columns before {min(b for b, _ in meds):.1f} - {max(b for b, _ in meds):.1f}, "
          f"after {min(a for _, a in meds):.1f} - {max(a for _, a in meds):.1f}")
    assert all(a < b for b, a in meds), meds


def test_consensus_rule_by_hand():
    """One pile row by hand: the depth's ends, a shallow column inside, insertions with and without a majority, ties, a deletion."""
    R = "ACGTACGTAC"
    pile = np.zeros((10, 13), np.int64)
    code = {"A": 0, "C": 1, "T": 2, "G": 3}
    for j in range(1, 9):
        pile[j, code[R[j]]] = 4
    pile[0, 0] = 2                                 # depth 2: in front of the first column
    pile[3, :] = 0
    pile[3, 1] = 2                                 # a shallow column inside: R's letter (T), whatever the two reads say
    pile[2, 5 + 2], pile[2, 9 + 3] = 3, 3          # 3 of 4 insert T, then G, in front of column 2
    pile[4, 5 + 1] = 2                             # 2 of 4 insert: no majority
    pile[5, :5] = [0, 2, 2, 0, 0]                  # a tie that holds R's own letter (C)
    pile[6, :5] = [2, 0, 2, 0, 0]                  # a tie without it: the smallest state
    pile[7, :5] = [0, 0, 1, 0, 3]                  # deleted
    for fn in (lambda: orc.consensus(pile, R, 3), lambda: _as_tuple(consensus.call_consensus(pile, [code[ch] for ch in R], 3))):
        letters, first, last, cpos = fn()
        assert (letters, first, last) == ("C" + "TG" + "G" + "T" + "A" + "C" + "A" + "A", 1, 8)
        assert list(cpos) == [-1, 0, 3, 4, 5, 6, 7, 8, 8, 9]
    c = consensus.call_consensus(pile, [code[ch] for ch in R], 3)
    assert (c["substituted"], c["deleted"], c["inserted"]) == (1, 1, 2) and c["depth"].tolist() == [4, 4, 2, 4, 4, 4, 4, 4]
    assert consensus.column_at(c, -5) == -6 and consensus.column_at(c, 12) == 12 and consensus.call_consensus(pile, [code[ch] for ch in R], 5) is None
    record, telo = consensus.reference_record("CCCTAA", "ACGT" * 500, 100, 6000)
    assert telo == 4104 and len(record) == 6004 and record.startswith("CCCTAA" * 684 + ("ACGT" * 500)[100:])
    assert consensus.reference_record("CCCTAA", "ACGT" * 500, 100, 6004)[1] == 4110          # (longer than --minSeqLength, not as long)
    assert consensus.reference_record("CCCTAA", "ACGT" * 500, -7, 0)[1] == 2502


def _as_tuple(c):
    return "".join(consensus.LETTERS[x] for x in c["codes"]), c["first"], c["last"], c["cpos"]


@pytest.fixture(scope="module")
def engine():
    import emu_align_driver
    import emu_anchor_driver
    emu_anchor_driver.build()
    emu_align_driver.build()
    from emu_align_engine import EmuAlignEngine
    return EmuAlignEngine()


@pytest.mark.parametrize("ident", ["CCCTAA_ONT", "AAACCCT_HIFI"])
def test_host_module_on_the_emulation_gives_the_oracles_consensus(engine, ident):
    """consensus.run behind anchor.run, both on the emulations: the letters, the columns, the reads' rows and the medians are the oracle's."""
    p = planted(ident)
    rows_ = ac.detection_rows(ident)
    g_end, links = ac.detection_groups(ident)
    n = len(g_end)
    rows = [("reads.fasta", f"read{i}", 0, int(rows_["begin"][i]), int(rows_["begin"][i]), int(rows_["begin"][i]) + ec.SPAN, 999, None, int(rows_["length"][i]),
             rows_["codes"][i], rows_["keep"][i]) for i in range(n)]
    read_rows = [["reads.fasta", f"read{i}", "forward", 0, 0, 0, 999, g_end[i], links[i], 0] for i in range(n)]
    a_reads, a_groups, _ = anchor.run(rows, read_rows, engine, ec.K, ec.SPAN)
    before = len(engine.align_calls) if hasattr(engine, "align_calls") else 0
    records, c_groups, c_reads, references, stats = consensus.run(rows, read_rows, a_reads, a_groups, engine, ident.rsplit("_", 1)[0], ec.SPAN, MIN_DEPTH, 5000)
    assert len(engine.align_calls) == before + 2 and engine.align_calls[-2] == (72, 6, 6) and engine.align_calls[-1] == (72, 6, 0)
    assert [letters for _h, letters in records] == [c[0] for c in p["cons"]] and len(records) == len(references) == 6
    assert stats["used"] == stats["anchored"] == 72 and stats["edge"] == 0 and stats["with_consensus"] == stats["groups"] == 6
    by_id = {r[1]: r for r in c_reads}
    for m, i in enumerate(p["members"]):
        assert by_id[f"read{i}"][3:] == [int(x) for x in p["stat1"][m, :5]] + [0, 1, int(p["stat2"][m, 0])]
    assert all(r[3:] == [""] * 8 for r in c_reads if g_end[int(r[1][4:])] == 0) and [r[1] for r in c_reads] == [r[1] for r in read_rows]
    for g, row in zip(p["groups"], c_groups):
        c = p["cons"][g - 1]
        assert row[:6] == [g, 12, 12, 12, 0, f"read{p['ref_read'][g]}"] and row[6:9] == [c[1], c[2], len(c[0])]
        header = records[g - 1][0].split()
        boundary = int(a_groups[g - 1][4]) - int(rows_["begin"][p["ref_read"][g]])
        # (a boundary in front of the reference's window: the columns go on at one letter each, the position is negative)
        at = c[3][0] + boundary if boundary < 0 else c[3][-1] + boundary - (len(c[3]) - 1) if boundary >= len(c[3]) else c[3][boundary]
        assert header[0] == f"end{g}" and header[4] == f"boundary={at}"
        rec = references[g - 1][1]
        unit = ident.rsplit("_", 1)[0]
        telo = len(rec) - len(c[0][max(at, 0):])
        assert telo % len(unit) == 0 and telo >= 2500 and len(rec) > 5000 and rec == unit * (telo // len(unit)) + c[0][max(at, 0):]
        if ident.endswith("_ONT"):
            assert float(row[15]) < float(row[14])
