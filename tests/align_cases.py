"""Test helper: the pairs of the banded alignment tests (tests/test_align.py on the host emulation, tests/test_gpu_align.py on the
GPU), the refusals of tps_window_align, and the oracle's answers, computed once per process (tests/align_oracle.py)."""
import functools

import numpy as np

import align_oracle as orc
import ends_cases as ec


class Case:
    """Queries and reference rows as strings; pair i = queries[i] against refs[ref[i]] on the diagonal centre[i], counted on pile row
    pile_row[i]."""

    def __init__(self, name, span, n_pile=1):
        self.name, self.span, self.n_pile = name, span, n_pile
        self.queries, self.refs, self.ref, self.centre, self.pile_row, self.notes = [], [], [], [], [], []

    def add_ref(self, r):
        self.refs.append(r)
        return len(self.refs) - 1

    def add(self, q, r, centre=0, pile_row=-1, note=""):
        """r: a string (a reference row of its own), a row's number, or None."""
        self.queries.append(q)
        self.ref.append(-1 if r is None else r if isinstance(r, int) else self.add_ref(r))
        self.centre.append(centre)
        self.pile_row.append(pile_row)
        self.notes.append(note)
        return len(self.queries) - 1


def _related(rng, n, m):
    """Two windows of n and m letters off one random string, a few edits apart."""
    base = ec.rand(rng, max(n, m) + 8 + max(n, m) // 16)
    q = ec.mutate(rng, base, (0.02, 0.01, 0.01))[:n]
    assert len(q) == n
    return q, base[:m]


def _hand_case():
    """The small pairs, span 300.  Pile row 0: the clean pairs of one reference; pile row 1: the pairs with inserted letters; the
    flagged pairs sit on pile rows too and must not count."""
    rng = np.random.default_rng(2401)
    c = Case("hand", 300, n_pile=3)
    R = ec.rand(rng, 120)
    r0 = c.add_ref(R)
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    c.add(R, r0, 0, 0, "equal windows")
    c.add(R[:60] + other[R[60]] + R[61:], r0, 0, 0, "one substitution")
    c.add(R[:40] + other[R[40]] + R[40:80] + R[81:], r0, 0, 0, "one inserted and one deleted letter")
    # (inserted letters that occur on neither side of their place: no other path costs as little)
    x, y = [ch for ch in "ACGT" if ch not in R[49] + R[50]][:2]
    two, four = x + y, 2 * "".join(ch for ch in "ACGT" if ch not in R[69] + R[70])[:2]
    assert R[49] != R[50] and R[69] != R[70] and len(four) == 4
    c.add(R[:50] + two + R[50:], r0, 0, 1, "two inserted letters")
    c.add(R[:70] + four + R[70:], r0, 0, 1, "four inserted letters: the cap of 3")
    c.add(R[:50] + two + R[50:70] + four + R[70:], r0, 0, 1, "both runs: ins1 and ins2 of one pile row")
    c.add(R[:50] + two[0] + R[50:], r0, 0, 1, "one inserted letter where two others have two")
    c.add(R[10:100], r0, 10, 0, "a query that starts and ends inside the reference")
    c.add(R[10:100], r0, 0, 0, "... with the band ten diagonals off")
    c.add(R, r0, 0, -1, "pile_row -1: not counted")
    # ties of the traceback: diagonal, then up, then left
    # (flanks longer than the band is wide: with both leading ends free, a window shorter than that ends on any letter that matches)
    F1, F2 = ec.rand(rng, 39) + "G", "T" + ec.rand(rng, 39)
    h = c.add_ref(F1 + "A" * 6 + F2)
    c.add(F1 + "A" * 7 + F2, h, 0, 2, "a homopolymer one letter longer")
    c.add(F1 + "A" * 5 + F2, h, 0, 2, "a homopolymer one letter shorter")
    c.add(F1 + "ACAC" + F2, F1 + "AC" + F2, 0, -1, "ACAC against AC between flanks")
    c.add(F1 + "AC" + F2, F1 + "ACAC" + F2, 0, -1, "AC against ACAC between flanks")
    c.add("ACAC", "AC", 0, -1, "ACAC against AC")
    c.add("AC", "ACAC", 0, -1, "AC against ACAC")
    c.add("ACAC", "AC", -2, -1, "ACAC against AC, the band two down")
    # several end cells of equal D: the largest i, then the largest j
    c.add("AAAA", "AAAAAAAA", 0, -1, "end cells of equal D on the last row and the last column")
    c.add("AAAAAAAA", "AAAA", 0, -1, "... with the longer query")
    c.add("ACGTACGT", "TTTTACGTACGTCCCC", 4, -1, "the query inside the reference")
    c.add("TTTTACGTACGTCCCC", "ACGTACGT", -4, -1, "the reference inside the query")
    # the band's edge: a run of extra letters pushes the path to lane 0 (query) or lane 63 (reference), then out of the band
    S = ec.rand(rng, 200)
    s0 = c.add_ref(S)
    for run in (30, 31, 32, 33):
        extra = ec.rand(rng, run)
        c.add(S[:100] + extra + S[100:], s0, 0, 0, f"{run} extra letters in the query")
        c.add(S[:100] + S[100 + run:], s0, 0, 0, f"{run} extra letters in the reference")
    # no reference; a row that is its own reference; letters read as A
    c.add(R, None, 0, 0, "ref < 0")
    c.add(R, None, 7, -1, "ref < 0 again")
    c.add(S, s0, 0, 2, "a row equal to its reference")
    N = R[:30] + "NNNN" + R[34:60] + "nryk" + R[64:]
    c.add(N, r0, 0, 0, "letters that are not ACGT in the query")
    c.add(R, N, 0, -1, "... in the reference")
    c.add("N" * 20, "A" * 20, 0, -1, "N against A")
    # centres that put the band partly and wholly beside the matrix
    for centre in (-4096, -300, -152, -151, -33, -32, -31, 0, 31, 32, 33, 151, 152, 153, 300, 4096):
        c.add(R, r0, centre, 0, f"centre {centre}")
    c.add("", r0, 0, 0, "an empty query")
    c.add(R, "", 0, 0, "an empty reference")
    c.add("", "", 0, -1, "both empty")
    c.add("", "", 1, -1, "both empty, the band beside them")
    return c


LENGTHS = (0, 1, 63, 64, 65, 4096)


def _lengths_case():
    rng = np.random.default_rng(2402)
    c = Case("lengths", 4096)
    for n in LENGTHS:
        for m in LENGTHS:
            q, r = _related(rng, n, m)
            c.add(q, r, 0, 0, f"{n} against {m}")
    q, r = _related(rng, 4096, 4096)
    for centre in (-4096, -4065, -4064, 4064, 4065, 4096):
        c.add(q, r, centre, -1, f"4096 against 4096, centre {centre}")
    return c


def _span_case(span):
    rng = np.random.default_rng(2403 + span)
    c = Case(f"span{span}", span)
    q, r = _related(rng, span, span)
    c.add(q, r, 0, 0, "full rows")
    c.add(r, r, 0, 0, "equal")
    c.add(q[: span // 2], r, 0, 0, "half a query")
    c.add(q, r[: span // 2], 1, -1, "half a reference")
    c.add("C" * span, "A" * span, 0, 0, "nothing in common")
    return c


@functools.lru_cache(maxsize=None)
def _planted_case(ident):
    """The 72 grouped reads of a planted set of tests/ends_cases.py, each against its group's reference read on the anchor's offset:
    the first pass of topsicle_amd/consensus.py."""
    import anchor_cases as ac
    import anchor_oracle as ao
    rows = ac.detection_rows(ident)
    offset, _votes, _second = ao.window_offsets(rows["windows"], rows["keeps"], rows["ref"], ec.K)
    members = [i for i in range(len(rows["ref"])) if rows["ref"][i] >= 0]
    refs = sorted({rows["ref"][i] for i in members})
    c = Case(f"planted_{ident}", ec.SPAN, n_pile=len(refs))
    for r in refs:
        c.add_ref(rows["windows"][r])
    for i in members:
        g = refs.index(rows["ref"][i])
        c.add(rows["windows"][i], g, int(offset[i]), g, f"read {i}")
    assert len(members) == ec.N_ENDS * ec.PER_END
    return c


PLANTED = ("CCCTAA_ONT", "ACGGATGTCTAACTTCTTGGTGT_HIFI")
CASE_IDS = ["hand", "lengths", "span1", "span17", "span4096"] + [f"planted_{p}" for p in PLANTED]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "hand":
        return _hand_case()
    if name == "lengths":
        return _lengths_case()
    if name.startswith("span"):
        return _span_case(int(name[4:]))
    return _planted_case(name[len("planted_"):])


@functools.lru_cache(maxsize=None)
def rows(name):
    """The arrays of the C call: dict(codes, length, ref_codes, ref_length, ref, centre, pile_row, span, n_pile)."""
    c = case(name)
    codes, length = orc.pack(c.queries, c.span)
    ref_codes, ref_length = orc.pack(c.refs, c.span)
    return dict(codes=codes, length=length, ref_codes=ref_codes, ref_length=ref_length, ref=np.array(c.ref, np.int32), centre=np.array(c.centre, np.int32),
                pile_row=np.array(c.pile_row, np.int32), span=c.span, n_pile=c.n_pile)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(stat, cols, pile) by the oracle; read-only."""
    c = case(name)
    out = orc.window_align(c.queries, c.refs, c.ref, c.centre, c.span, c.pile_row, c.n_pile)
    for a in out:
        a.setflags(write=False)
    return out


def assert_equal(got, name, cols=True, pile=True):
    """stat, cols and pile bit for bit; a piece that was not asked for is None."""
    c = case(name)
    stat, want_cols, want_pile = expected(name)
    for i in np.flatnonzero((got[0] != stat).any(axis=1))[:1]:
        raise AssertionError(f"{name} pair {i} ({c.notes[i]}): stat {got[0][i].tolist()}, want {stat[i].tolist()}")
    if cols:
        for i in np.flatnonzero((got[1] != want_cols).any(axis=1))[:1]:
            j = int(np.flatnonzero(got[1][i] != want_cols[i])[0])
            raise AssertionError(f"{name} pair {i} ({c.notes[i]}): column {j} is {got[1][i, j]}, want {want_cols[i, j]}")
    else:
        assert got[1] is None
    if pile:
        assert got[2].shape == want_pile.shape and got[2].dtype == np.int32
        for p, j, e in np.argwhere(got[2] != want_pile)[:1]:
            raise AssertionError(f"{name} pile row {p} column {j} entry {e}: {got[2][p, j, e]}, want {want_pile[p, j, e]}")
    else:
        assert got[2] is None


def run_case(align_windows, name, cols=True, pile=True):
    """`align_windows` has HipScanner.align_windows' signature."""
    r = rows(name)
    return align_windows(r["codes"], r["length"], r["ref_codes"], r["ref_length"], r["ref"], r["centre"], r["span"], cols=cols,
                         pile_row=r["pile_row"] if pile else None, n_pile=r["n_pile"] if pile else 0)


# ---- the refusals: what differs from GOOD, the code, the message.  `lens` = (codes_len, ref_codes_len, stat_len, cols_len, pile_len)
# where they are not what the arrays say; `null` = arrays handed over as NULL.
GOOD = dict(n=2, n_ref=3, span=100, n_pile=2, length=[100, 5], ref_length=[100, 0, 50], ref=[1, -7], centre=[0, -4096], pile_row=[1, -1], lens=None, null=())
GOOD_LENS = (14, 21, 12, 200, 2600)
REFUSALS = [
    (dict(n=262145, lens=(262145 * 7, 21, 262145 * 6, 262145 * 100, 2600)), -5, "n must be 0..262144"),
    (dict(n=-1, lens=(-7, 21, -6, -100, 2600)), -5, "n must be 0..262144"),
    (dict(n_ref=0, lens=(14, 0, 12, 200, 2600)), -5, "n_ref must be 1..262144"),
    (dict(n_ref=262145, lens=(14, 262145 * 7, 12, 200, 2600)), -5, "n_ref must be 1..262144"),
    (dict(span=0, lens=(0, 0, 12, 0, 0)), -5, "span must be 1..4096"),
    (dict(span=4097, lens=(514, 771, 12, 8194, 2 * 4097 * 13)), -5, "span must be 1..4096"),
    (dict(n_pile=-1), -5, "n_pile must be 0..n_ref"),
    (dict(n_pile=4, lens=(14, 21, 12, 200, 5200)), -5, "n_pile must be 0..n_ref"),
    (dict(lens=(13, 21, 12, 200, 2600)), -3, "codes must hold 14 dwords"),
    (dict(lens=(14, 20, 12, 200, 2600)), -3, "ref_codes must hold 21 dwords"),
    (dict(lens=(14, 21, 11, 200, 2600)), -3, "stat must hold 12 entries"),
    (dict(lens=(14, 21, 12, 199, 2600)), -3, "cols must hold 200 entries"),
    (dict(lens=(14, 21, 12, 200, 2600), null=("cols",)), -3, "cols must hold 0 entries"),
    (dict(lens=(14, 21, 12, 200, 2599)), -3, "pile must hold 2600 entries"),
    (dict(lens=(14, 21, 12, 200, 2600), null=("pile",)), -3, "pile must hold 0 entries"),
    (dict(n_pile=0, lens=(14, 21, 12, 200, 0)), -3, "a pile needs n_pile of 1 or more"),
    (dict(null=("pile_row",)), -3, "n_pile rows need pile_row"),
    (dict(null=("codes",)), -3, "null codes / length / ref_codes / ref_length / ref / centre / stat"),
    (dict(null=("stat",)), -3, "null codes / length / ref_codes / ref_length / ref / centre / stat"),
    (dict(ref_length=[100, 101, 50]), -3, "reference row 1: length must be 0..span"),
    (dict(ref_length=[100, 0, -1]), -3, "reference row 2: length must be 0..span"),
    (dict(length=[101, 5]), -3, "row 0: length must be 0..span"),
    (dict(length=[100, -1]), -3, "row 1: length must be 0..span"),
    (dict(ref=[3, -7]), -3, "row 0: ref must be below n_ref (negative: no reference)"),
    (dict(centre=[4097, 0]), -3, "row 0: centre must be -4096..4096"),
    (dict(centre=[0, -4097]), -3, "row 1: centre must be -4096..4096"),
    (dict(pile_row=[2, -1]), -3, "row 0: pile_row must be below n_pile (negative: not counted)"),
]
REFUSAL_IDS = [f"{i}_{msg.split(':')[-1].strip().replace(' ', '_')[:28]}" for i, (_kw, _rc, msg) in enumerate(REFUSALS)]


def refusal_call(raw, **kw):
    """GOOD with `kw` over it through `raw` (the C call's own argument list behind a context, every length as given): (rc, stat,
    cols, pile)."""
    p = dict(GOOD, **kw)
    n_rows, n_refs = len(p["length"]), len(p["ref_length"])
    cdw = 7
    arr = dict(codes=np.zeros((n_rows, cdw), np.uint32), length=np.array(p["length"], np.int32), ref_codes=np.zeros((n_refs, cdw), np.uint32),
               ref_length=np.array(p["ref_length"], np.int32), ref=np.array(p["ref"], np.int32), centre=np.array(p["centre"], np.int32),
               stat=np.full((n_rows, 6), 99, np.int32), cols=np.full((n_rows, 100), 99, np.uint16), pile_row=np.array(p["pile_row"], np.int32),
               pile=np.full((2, 100, 13), 99, np.int32))
    a = {k: (None if k in p["null"] else v) for k, v in arr.items()}
    lens = p["lens"] if p["lens"] is not None else GOOD_LENS
    rc = raw(a["codes"], lens[0], a["length"], p["n"], a["ref_codes"], lens[1], a["ref_length"], p["n_ref"], a["ref"], a["centre"], p["span"], a["stat"], lens[2],
             a["cols"], lens[3], a["pile_row"], a["pile"], p["n_pile"], lens[4])
    return rc, arr["stat"], arr["cols"], arr["pile"]
