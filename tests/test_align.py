"""Windows aligned base by base (tps_window_align; csrc/tps_align.h) on the host emulation of the kernel: stat, cols and pile equal
to the plain restatement of the rule on strings (tests/align_oracle.py) bit for bit, the refusals with the library's codes and
words, and the same kernel text as a program of its own under the sanitizers.  tests/test_gpu_align.py asks the library the same."""
import subprocess

import numpy as np
import pytest

import align_cases as ac
import align_oracle as orc
import emu_align_driver as emu
from topsicle_amd import hiplib


@pytest.mark.parametrize("name", ac.CASE_IDS)
def test_emulation_equals_oracle(name):
    ac.assert_equal(ac.run_case(emu.window_align, name), name)


@pytest.mark.parametrize("cols,pile", [(False, True), (True, False), (False, False)])
def test_pieces_not_asked_for(cols, pile):
    """cols NULL, pile NULL, both: the other outputs are what they are with everything asked for."""
    for name in ("hand", "span17"):
        ac.assert_equal(ac.run_case(emu.window_align, name, cols=cols, pile=pile), name, cols=cols, pile=pile)


def test_cases_reach_what_they_are_for():
    """The edge cases say what they claim to say (on the oracle's answers)."""
    c = ac.case("hand")
    stat, cols, pile = ac.expected("hand")
    at = {note: i for i, note in enumerate(c.notes)}
    R = c.refs[0]

    def row(note):
        return stat[at[note]].tolist()
    assert row("equal windows") == [0, 0, 120, 0, 120, 0] and row("one substitution") == [1, 0, 120, 0, 120, 0]
    assert row("one inserted and one deleted letter") == [2, 0, 120, 0, 120, 0]
    i = at["one inserted and one deleted letter"]
    assert (cols[i] >> 3 & 3).sum() == 1 and (cols[i] & 7 == orc.DELETED).sum() == 1 and (cols[i, 120:] == orc.UNCOVERED).all()
    i2, i4 = at["two inserted letters"], at["four inserted letters: the cap of 3"]
    assert stat[i2, 0] == 2 and stat[i4, 0] == 4 and sorted(cols[i2] >> 3 & 3)[-2:] == [0, 2] and sorted(cols[i4] >> 3 & 3)[-2:] == [0, 3]
    j2, j4 = int(np.argmax(cols[i2] >> 3 & 3)), int(np.argmax(cols[i4] >> 3 & 3))
    q2, q4 = c.queries[i2], c.queries[i4]
    assert [orc.LETTERS[cols[i2, j2] >> 5 & 3], orc.LETTERS[cols[i2, j2] >> 7 & 3]] == list(q2[j2:j2 + 2]) and q2[j2 + 2:] == R[j2:]
    assert [orc.LETTERS[cols[i4, j4] >> 5 & 3], orc.LETTERS[cols[i4, j4] >> 7 & 3]] == list(q4[j4:j4 + 2]) and q4[j4 + 4:] == R[j4:]
    # pile row 1: four pairs; ins1 counted by all that insert there, ins2 only by those with two letters or more
    assert pile[1, j2, 5:9].sum() == 3 and pile[1, j2, 9:13].sum() == 2 and pile[1, j4, 5:9].sum() == 2 and pile[1, j4, 9:13].sum() == 2
    assert (pile[1, :120, :5].sum(axis=1) == 4).all() and (pile[1, 120:] == 0).all()
    assert row("a query that starts and ends inside the reference") == [0, 0, 90, 10, 100, 0] == row("... with the band ten diagonals off")
    # the tie order: diagonal, then up, then left -- the extra letter of a run is the run's first, the missing one too
    h = at["a homopolymer one letter longer"]
    assert stat[h].tolist() == [1, 0, 87, 0, 86, 0] and np.flatnonzero(cols[h] >> 3).tolist() == [40] and cols[h, 40] == 0 | 1 << 3 | 0 << 5
    h = at["a homopolymer one letter shorter"]
    assert stat[h].tolist() == [1, 0, 85, 0, 86, 0] and np.flatnonzero(cols[h] == orc.DELETED).tolist() == [40]
    h = at["ACAC against AC between flanks"]          # the FIRST "AC" is the inserted one: A, then C, in front of the reference's A
    assert stat[h].tolist() == [2, 0, 84, 0, 82, 0] and np.flatnonzero(cols[h] >> 3).tolist() == [40] and cols[h, 40] == 0 | 2 << 3 | 0 << 5 | 1 << 7
    h = at["AC against ACAC between flanks"]          # ... and the first "AC" the deleted one
    assert stat[h].tolist() == [2, 0, 82, 0, 84, 0] and np.flatnonzero(cols[h] == orc.DELETED).tolist() == [40, 41]
    # short windows: both leading ends are free, so the path may be the last letters alone
    assert row("ACAC against AC") == [0, 2, 4, 0, 2, 0] == row("ACAC against AC, the band two down") and row("AC against ACAC") == [0, 0, 2, 2, 4, 0]
    # equal D on many end cells: the largest i, then the largest j
    assert row("end cells of equal D on the last row and the last column") == [0, 0, 4, 4, 8, 0] and row("... with the longer query") == [0, 4, 8, 0, 4, 0]
    assert row("the query inside the reference") == [0, 0, 8, 4, 12, 0] and row("the reference inside the query") == [0, 16, 16, 0, 0, 0]
    # the band's edge: lane 0 is the diagonal centre - 32, lane 63 centre + 31.  30 letters fit, the 32nd extra letter of a query and
    # the 31st of a reference put the path on the edge, one more and the band cannot hold it
    for note, dist, flags in (("30 extra letters in the query", 30, 0), ("31 extra letters in the query", 31, 0), ("32 extra letters in the query", 32, orc.EDGE),
                              ("30 extra letters in the reference", 30, 0), ("31 extra letters in the reference", 31, orc.EDGE)):
        assert row(note)[0] == dist and row(note)[3:] == [0, 200, flags], note
    for note, run in (("33 extra letters in the query", 33), ("32 extra letters in the reference", 32), ("33 extra letters in the reference", 33)):
        assert row(note)[1:5] != [0, len(c.queries[at[note]]), 0, 200], note               # (no path through both windows whole)
    assert row("ref < 0") == [0, 0, 0, 0, 0, orc.NONE] and (cols[at["ref < 0"]] == orc.UNCOVERED).all()
    assert row("a row equal to its reference") == [0, 0, 200, 0, 200, 0]
    assert row("letters that are not ACGT in the query")[0] == sum(R[j] != "A" for j in list(range(30, 34)) + list(range(60, 64))) > 0
    assert row("N against A") == [0, 0, 20, 0, 20, 0]
    # centres: the band wholly beside the matrix is NONE; its last cell on either side is a corner of the matrix
    for centre, flags in ((-4096, orc.NONE), (-152, orc.NONE), (-151, 0), (0, 0), (152, 0), (153, orc.NONE), (4096, orc.NONE)):
        assert row(f"centre {centre}")[5] == flags, centre
    assert row("centre -151") == [0, 120, 120, 0, 0, 0] and row("centre 152") == [0, 0, 0, 120, 120, 0]
    assert row("centre 31") == row("centre 0") == [0, 0, 120, 0, 120, 0] and row("centre -31") == row("centre 32") == [0, 0, 120, 0, 120, orc.EDGE]
    assert row("centre -32")[0] > 0 and row("centre 33")[0] > 0                               # (the main diagonal is outside)
    assert row("an empty query") == [0, 0, 0, 31, 31, 0] and row("an empty reference") == [0, 32, 32, 0, 0, 0]
    assert row("both empty") == [0, 0, 0, 0, 0, 0] and row("both empty, the band beside them") == [0, 0, 0, 0, 0, 0]
    # flagged pairs and pile_row -1 do not count: pile row 0 holds the unflagged pairs of its rows only
    mine = [i for i in range(len(c.ref)) if c.pile_row[i] == 0 and stat[i, 5] == 0]
    assert len(mine) < sum(p == 0 for p in c.pile_row) and sum(int(stat[i, 4] - stat[i, 3]) for i in mine) == pile[0, :, :5].sum()
    # the lengths against each other, the spans, the far centres
    L = ac.case("lengths")
    assert [(len(q), len(L.refs[r])) for q, r in zip(L.queries[:36], L.ref[:36])] == [(n, m) for n in ac.LENGTHS for m in ac.LENGTHS]
    ls = ac.expected("lengths")[0]
    assert (ls[:36, 5] & orc.NONE == 0).all() and ls[35, 0] > 50 and ls[35, 2] == 4096
    assert ls[36].tolist() == [0, 4096, 4096, 0, 0, 0] and ls[41].tolist() == [0, 0, 0, 4096, 4096, 0]
    assert {ac.case(n).span for n in ac.CASE_IDS} >= {1, 17, 4096}
    for p in ac.PLANTED:
        ps = ac.expected(f"planted_{p}")[0]
        assert len(ps) == 72 and (ps[:, 5] == 0).all() and (ps[:, 4] - ps[:, 3] > 1000).all()


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("align_cases") / "cases.txt"
    with open(path, "w") as fh:
        for name in ac.CASE_IDS:
            c = ac.case(name)
            fh.write(f"acase {c.span} {len(c.refs)} {len(c.queries)} {c.n_pile}\n")
            fh.write("".join(f"{r or '-'}\n" for r in c.refs))
            fh.write("".join(f"{ref} {centre} {prow} {q or '-'}\n" for q, ref, centre, prow in zip(c.queries, c.ref, c.centre, c.pile_row)))
    return str(path)


def test_standalone_program_is_clean_under_sanitizers(cases_file):
    """The same kernel text under -fsanitize=address,undefined, as a program of its own, on the cases of this file: poisoned LDS of
    exactly one wave's size, rows of exactly their sizes; every pair checked against the program's own cell-by-cell restatement of
    the rule, with cols and pile asked for and not.  Then its built-in batch."""
    exe = emu.build_main()
    for argv in ([exe, cases_file], [exe]):
        out = subprocess.run(argv, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert out.stdout.startswith("ok 4 cases")


@pytest.mark.parametrize("kw,code,msg", ac.REFUSALS, ids=ac.REFUSAL_IDS)
def test_refusals_carry_the_librarys_codes(kw, code, msg):
    """TPS_E_ARG (-3) and TPS_E_CAPACITY (-5) as tps_window_align returns them, with its words (test_gpu_align.py asks the library the
    same); a refused call writes nothing."""
    seen = []

    def raw(*args):
        rc, text = emu.window_align_raw(*args)
        seen.append(text)
        return rc
    rc, stat, cols, pile = ac.refusal_call(raw)
    assert rc == 0 and stat[:, 5].tolist() == [0, hiplib.ALIGN_NONE] and (cols == hiplib.ALIGN_UNCOVERED).all() and (pile == 0).all()
    rc, stat, cols, pile = ac.refusal_call(raw, **kw)
    assert (rc, seen[-1]) == (code, msg)
    assert (stat == 99).all() and (cols == 99).all() and (pile == 99).all()


def test_an_empty_call_clears_the_pile():
    pile = np.full((2, 100, 13), 5, np.int32)
    rc, _ = emu.window_align_raw(None, 0, None, 0, None, 21, None, 3, None, None, 100, None, 0, None, 0, np.zeros(1, np.int32), pile, 2, pile.size)
    assert rc == 0 and (pile == 0).all()
