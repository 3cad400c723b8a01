"""Test helper: the reads, windows and hand-built window sets of the anchoring tests (tests/test_anchor.py on the host emulation,
tests/test_gpu_ends_anchor.py on the GPU), the planted-end detection pipeline, and the oracle's answers to all of them, computed once per
process (tests/anchor_oracle.py)."""
import functools

import numpy as np

import anchor_oracle as orc
import ends_cases as ec
import ends_oracle as eo
from topsicle_amd import hiplib
from topsicle_amd.variants import unit_code
from tract_cases import repeats

UNITS = ec.UNITS


class Case:
    """Reads and windows for the extraction (`reads` ... `end`), or windows as strings with their kept sets (`windows`, `keeps`); `ref`
    for the offsets over the rows of either."""

    def __init__(self, name, unit="CCCTAA", k=12, span=2000):
        self.name, self.unit, self.k, self.span = name, unit, k, span
        self.reads, self.tails, self.begin, self.end, self.ref = [], [], [], [], []
        self.windows, self.keeps = None, None

    def add(self, molecule, tail, begin, end, ref=-1):
        """`molecule` is telomere first; tail 1 stores its reverse complement."""
        self.reads.append(ec.stored_revcomp(molecule) if tail else molecule)
        self.tails.append(tail)
        self.begin.append(begin)
        self.end.append(end)
        self.ref.append(ref)
        return len(self.reads) - 1

    def add_window(self, win, kept=None, ref=-1):
        """A window by hand: its letters and its kept positions (every position with k letters where none are given)."""
        if self.windows is None:
            self.windows, self.keeps = [], []
        self.windows.append(win)
        self.keeps.append(set(range(max(0, len(win) - self.k + 1))) if kept is None else set(kept))
        self.ref.append(ref)
        return len(self.windows) - 1

    @property
    def by_hand(self):
        return self.windows is not None


LENGTHS = (0, 11, 12, 63, 64, 65, 3968, 3969, 3979, 3980, 4096)          # (k = 12: k - 1, k; one piece, its seam, two pieces)


def _lengths_case():
    """Windows of 0, k - 1, k, 63, 64, 65 ... 4096 letters on both tails, begun 20 bases inside the repeat (the first keep bits are
    clear); a repeat word lies over the seam of the kernel's two pieces.  Every row against the longest window of its tail."""
    rng = np.random.default_rng(201)
    c = Case("lengths", span=4096)
    s = list(repeats("CCCTAA", 300) + ec.rand(rng, 5000))
    s[280 + 3964:280 + 3970] = "CCCTAA"
    s[280 + 3975:280 + 3981] = "TTAGGG"
    mol = "".join(s)
    for tail in (0, 1):
        first = len(c.reads)
        for n in LENGTHS:
            c.add(mol, tail, 280, 280 + n, first + len(LENGTHS) - 1)
    c.ref[0] = -1
    c.ref[len(LENGTHS) - 1] = len(LENGTHS) - 1     # its own reference
    return c


def _past_end_case():
    """end past the read (clamped), begin past the read, an empty read; both tails; shifted windows of one molecule against each
    other."""
    rng = np.random.default_rng(202)
    c = Case("past_end")
    mol = ec.clean_random(rng, 1000, "CCCTAA")
    for tail in (0, 1):
        first = len(c.reads)
        c.add(mol, tail, 600, 2600, first)         # 400 letters
        c.add(mol, tail, 563, 2000, first)         # the same molecule 37 bases earlier: offset -37
        c.add(mol, tail, 700, 1000, first)
        c.add(mol, tail, 1200, 1300, first)        # begin past the read: no letters
        c.add(mol, tail, 989, 2989, first)         # k - 1 letters after the clamp
        c.add(mol, tail, 0, 0, first)
    c.reads.append("")                             # (no molecule: the empty read as stored)
    c.tails.append(0)
    c.begin.append(0)
    c.end.append(0)
    c.ref.append(0)
    return c


def _letters_case():
    """N and other letters, lower case, inside the window; both tails.  The clean copy is the reference."""
    rng = np.random.default_rng(203)
    c = Case("letters", span=1000)
    base = repeats("CCCTAA", 100) + ec.rand(rng, 900)
    for tail in (0, 1):
        first = len(c.reads)
        c.add(base, tail, 50, 1000, first)
        s = list(base)
        for p in (120, 121, 300, 511, 512, 999):
            s[p] = "N"
        s[700] = "R"
        c.add("".join(s), tail, 50, 1000, first)
        c.add(base.lower(), tail, 50, 1000, first)
        c.add("".join(ch.lower() if i % 3 else ch for i, ch in enumerate(s)), tail, 60, 1000, first)
        c.add("N" * 400, tail, 0, 400, first)
    return c


def _unit_case(key, k=12, span=2000, name=None):
    """Three molecules -- 300 bases of telomere, then random subtelomere -- each on tail 0, on tail 1 begun 37 bases later and on tail
    0 begun 100 bases earlier; the first is the reference of the three, and one row is set against another molecule."""
    unit = UNITS[key]
    rng = np.random.default_rng(300 + len(unit) + k + span)
    c = Case(name or f"unit_{key}", unit, k, span)
    for i in range(3):
        mol = repeats(unit, 300, i) + ec.rand(rng, 2100 + 37 * i)
        first = len(c.reads)
        c.add(mol, 0, 290 + i, 290 + i + span - 40, first)
        c.add(mol, 1, 327 + i, 327 + i + span, first)
        c.add(mol, 0, 190 + i, 190 + i + span, first if i else -1)
    c.ref[5] = 0                                   # another molecule's window: no votes
    return c


def _span_case(span):
    """A span that is no multiple of 16 or 32, and the smallest one (span = k): rows of one or two dwords."""
    rng = np.random.default_rng(400 + span)
    c = Case(f"span{span}", span=span)
    mol = ec.clean_random(rng, 400, "CCCTAA")
    for tail in (0, 1):
        first = len(c.reads)
        c.add(mol, tail, 100, 100 + span, first)
        c.add(mol, tail, 100 + span // 3, 100 + span // 3 + span, first)
        c.add(mol, tail, 120, 120 + span - 1, first)
    return c


def _kmers_of_one_slot(k):
    """Two k-mers whose hashes share the top 12 bits: (the one with the smaller low 20 bits, the other)."""
    rng = np.random.default_rng(500 + k)
    seen = {}
    while True:
        s = ec.rand(rng, k)
        x = eo.kmer_hash(s)
        other = seen.setdefault(x >> 20, s)
        if other != s and (eo.kmer_hash(other) & 0xFFFFF) != (x & 0xFFFFF):
            return tuple(sorted((s, other), key=lambda t: eo.kmer_hash(t) & 0xFFFFF))


def _table_case():
    """A reference with a duplicated k-mer (the smaller q wins), two k-mers of one slot (the smaller low 20 bits win, the loser never
    votes, and votes where it is alone), no vote at all, a row without a reference."""
    rng = np.random.default_rng(204)
    c = Case("table", span=300)
    s = list(ec.rand(rng, 300))
    s[200:212] = s[50:62]
    r = c.add_window("".join(s), ref=0)
    c.add_window("".join(s[50:62]), ref=r)         # one vote for d = 50, not 200
    c.add_window("".join(s[195:215]), kept={5}, ref=r)
    lo, hi = _kmers_of_one_slot(12)
    for first, second in ((lo, hi), (hi, lo)):     # (the order in the reference does not matter)
        r2 = c.add_window(first + second, kept={0, 12}, ref=-1)
        c.add_window("ACGT" + lo, kept={4}, ref=r2)
        c.add_window("ACGT" + hi, kept={4}, ref=r2)     # the loser: no vote
    r3 = c.add_window(hi, ref=-1)
    c.add_window("ACGT" + hi, kept={4}, ref=r3)    # alone in its slot it votes
    c.add_window(ec.rand(rng, 300), ref=0)         # unrelated: no vote (or a chance one)
    c.add_window("".join(s), kept=set(), ref=0)    # no kept position
    c.add_window("".join(s[:11]), ref=0)           # shorter than k
    c.add_window("", ref=0)
    return c


def _edges_case():
    """Votes exactly on a coarse-bin edge (d = 64 c - 4096) and one less, on both sides of 0, and split over an edge."""
    rng = np.random.default_rng(205)
    c = Case("bin_edges", span=1500)
    R = ec.rand(rng, 1500)
    c.add_window(R, ref=0)
    for d in (64, 63, 128, 127, 1):
        c.add_window(R[d:d + 400], ref=0)
    for d in (64, 65, 63, 1):
        c.add_window(ec.rand(rng, d) + R[:400], ref=0)          # d negative
    c.add_window(R[64:200] + R[199:335], ref=0)    # 64 and 63: two bins of one pair
    c.add_window(R[128:264] + R[263 - 64:399 - 64], ref=0)     # 128 and 63
    return c


def _extreme_case(k):
    """The extreme diagonals d = +-(4096 - k): the reference's last k-mer is the query's first, and the other way round."""
    rng = np.random.default_rng(206 + k)
    c = Case(f"extreme_k{k}", k=k, span=4096)
    R = ec.rand(rng, 4096)
    c.add_window(R, kept={4096 - k}, ref=1)
    c.add_window(R[4096 - k:] + ec.rand(rng, 4096 - k), kept={0}, ref=0)
    return c


def _trim(c, R, Q, keep_by_d):
    """kept positions of Q that vote against R for the diagonals of keep_by_d {d: how many}, chosen from the votes the oracle counts"""
    table = orc.table_of(R, set(range(len(R) - c.k + 1)), c.k)
    kept, left = set(), dict(keep_by_d)
    for p in range(len(Q) - c.k + 1):
        ds = orc.diagonals(table, Q, {p}, c.k)
        if ds and left.get(ds[0], 0) > 0:
            left[ds[0]] -= 1
            kept.add(p)
    assert not any(left.values()), left
    return kept


def _median_case():
    """Two equal pair maxima (the smaller c wins, the other is `second`), and even numbers of votes (the lower median)."""
    rng = np.random.default_rng(207)
    c = Case("median", span=1000)
    R = ec.rand(rng, 1000)
    c.add_window(R, ref=-1)
    Q = R[500:560] + R[100:160]                    # d = 500 and d = 40
    c.add_window(Q, _trim(c, R, Q, {500: 30, 40: 30}), ref=0)
    c.add_window(Q, _trim(c, R, Q, {500: 31, 40: 30}), ref=0)
    Q = R[100:150] + "AC" + R[150:200]             # d = 100 and, behind the insertion, d = 98
    for n in (1, 2, 3):
        c.add_window(Q, _trim(c, R, Q, {100: n, 98: n}), ref=0)
    c.add_window(Q, _trim(c, R, Q, {100: 3, 98: 2}), ref=0)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    out = [_lengths_case(), _past_end_case(), _letters_case()]
    out += [_unit_case(key) for key in UNITS]
    out += [_unit_case("CCCTAA", 8, 1999, "k8_span1999"), _unit_case("CCCTAA", 16, 2001, "k16_span2001"), _unit_case("albicans23", 16, 777, "albicans23_k16_span777")]
    out += [_span_case(12), _span_case(33), _span_case(65)]
    out += [_table_case(), _edges_case(), _extreme_case(8), _extreme_case(12), _extreme_case(16), _median_case(), Case("empty")]
    return tuple(out)


CASE_IDS = [c.name for c in cases()]
WINDOW_IDS = [c.name for c in cases() if not c.by_hand]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """What the oracle says to case `name`: dict(codes, keep, length, windows, keeps, offsets=(offset, votes, second))."""
    c = case(name)
    if c.windows is not None:
        windows, keeps = c.windows, c.keeps
        codes, keep, _ = orc.pack(windows, keeps, c.span)
    else:
        codes, keep, windows, keeps = orc.end_window(c.reads, c.unit, c.tails, c.begin, c.end, c.k, c.span)
    length = np.array([len(w) for w in windows], np.int32)
    return dict(codes=codes, keep=keep, length=length, windows=windows, keeps=keeps, offsets=orc.window_offsets(windows, keeps, c.ref, c.k))


def assert_rows_equal(got, name):
    want = expected(name)
    for what, g in zip(("codes", "keep"), got):
        w = want[what]
        assert g.shape == w.shape and g.dtype == w.dtype, (name, what, g.shape, w.shape, g.dtype)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{name}: {what} differs at {bad[:5].tolist()}: got {g[tuple(bad[0])]:#x}, want {w[tuple(bad[0])]:#x}"


def assert_offsets_equal(got, name):
    want = expected(name)["offsets"]
    for what, g, w in zip(("offset", "votes", "second"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, what, g.shape, w.shape, g.dtype)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, f"{name}: {what} differs at rows {bad[:5].tolist()}: got {g[bad[0]]}, want {w[bad[0]]}"


def popcount(rows):
    return np.array([sum(bin(int(x)).count("1") for x in row) for row in rows], np.uint32)


# ---- the refusals: (what differs from a good call, the return code in the message)
U6 = unit_code("CCCTAA")[0]
WINDOW_REFUSALS = [
    (dict(code=unit_code("CCT")[0], m=3), "rc=-3"), (dict(code=unit_code("CCACCA")[0]), "rc=-3"), (dict(tails=[2]), "rc=-3"), (dict(begin=[-1]), "rc=-3"),
    (dict(begin=[50], end=[49]), "rc=-3"), (dict(lens=(2, 7, 4)), "rc=-3"), (dict(lens=(1, 6, 4)), "rc=-3"), (dict(lens=(1, 7, 3)), "rc=-3"),
    (dict(k=7), "rc=-5"), (dict(k=17), "rc=-5"), (dict(span=11), "rc=-5"), (dict(span=4097), "rc=-5"), (dict(begin=[0], end=[101]), "rc=-5"),
    (dict(span=4096, lens=(1, 256, 128), begin=[0], end=[16385]), "rc=-5"),
]
WINDOW_GOOD = dict(code=U6, m=6, tails=[0], begin=[0], end=[100], k=12, span=100, lens=None)          # rows of 7 and 4 dwords
OFFSET_REFUSALS = [
    (dict(n=262145, out_len=262145), "rc=-5"), (dict(span=11), "rc=-5"), (dict(span=4097), "rc=-5"), (dict(k=7), "rc=-5"), (dict(k=17), "rc=-5"),
    (dict(ref=[2, 0]), "rc=-3"), (dict(length=[101, 5]), "rc=-3"), (dict(length=[-1, 5]), "rc=-3"), (dict(out_len=1), "rc=-3"),
]
OFFSET_GOOD = dict(length=[100, 5], ref=[1, -7], span=100, k=12, n=None, out_len=None)


# ---- detection: planted chromosome ends, anchored
MIN_VOTES, RATIO = 20, 4                           # the defaults of topsicle_amd.anchor
BOUNDS = {"ONT": (40, 80), "HIFI": (10, 20)}       # pairwise error of anchored differences within an end: (p95, max)


@functools.lru_cache(maxsize=None)
def detection_groups(ident):
    """(end per read, links per read) of the planted set by the oracle's sketches and links and the grouping rule at its defaults: the
    `end` and `links` columns of end_reads_{k}.csv."""
    reads, _truth, tails, _telo = ec.detection_reads(ident)
    begin, end = ec.detection_windows(ident)
    motif = ident.rsplit("_", 1)[0]
    sketch, kept = eo.end_sketch(reads, motif, tails, begin, end, ec.K, ec.BUCKETS)
    part = [i for i in range(len(reads)) if kept[i] >= ec.MIN_KMERS]
    _degree, links, _ = eo.sketch_links(sketch[part], ec.MIN_MATCH, ec.MAX_LINKS)
    edges = [(i, int(j)) for i in range(len(part)) for j in links[i] if j >= 0]
    g_end, n_links = [0] * len(reads), [0] * len(reads)
    for p, g in zip(part, eo.groups(len(part), edges, ec.MIN_READS)):
        g_end[p] = g
    for i, j in edges:
        n_links[part[i]] += 1
        n_links[part[j]] += 1
    return g_end, n_links


@functools.lru_cache(maxsize=None)
def detection_rows(ident):
    """The oracle's windows of the planted set: dict(codes, keep, length, windows, keeps, begin, ref), ref by the host rule."""
    reads, _truth, tails, _telo = ec.detection_reads(ident)
    begin, end = ec.detection_windows(ident)
    motif = ident.rsplit("_", 1)[0]
    codes, keep, windows, keeps = orc.end_window(reads, motif, tails, begin, end, ec.K, ec.SPAN)
    g_end, n_links = detection_groups(ident)
    return dict(codes=codes, keep=keep, length=np.array([len(w) for w in windows], np.int32), windows=windows, keeps=keeps, begin=begin,
                ref=orc.references(g_end, n_links))


def detection_errors(ident, end, ref, begin, offset, votes, second):
    """The claim on a planted set, from the offsets of any engine: every planted read is anchored at the defaults; returns the sorted
    pairwise errors of the anchored differences against the planted ones within each planted end, and those of the called boundaries."""
    _reads, truth, _tails, telo = ec.detection_reads(ident)
    per_read, _cons = orc.anchor(end, ref, begin, begin, offset, votes, second, MIN_VOTES, RATIO)          # (the called length is the window's begin)
    anchored_err, called_err = [], []
    for e in range(1, ec.N_ENDS + 1):
        mine = [i for i in range(len(truth)) if truth[i] == e]
        assert all(end[i] == end[mine[0]] != 0 for i in mine), f"{ident}: planted end {e} is not one group"
        assert all(per_read[i] is not None for i in mine), f"{ident}: a read of planted end {e} is not anchored"
        anchored_err += orc.pair_errors([per_read[i][1] for i in mine], [telo[i] for i in mine])
        called_err += orc.pair_errors([begin[i] for i in mine], [telo[i] for i in mine])
    return sorted(anchored_err), sorted(called_err)


# ---- `--ends --anchor` end to end: what the CLI tests (host emulation and GPU) check
def _rows(path):
    import csv
    return list(csv.reader(open(path)))


def check_cli_outputs(outdir, ident, k=4):
    """anchored_reads_{k}.csv and anchored_ends_{k}.csv say what the planted set asks for: the headers, one row per row of
    end_reads_{k}.csv in its order, a reference of the read's own group, anchored_ends the summary of anchored_reads.  Returns the
    sorted pairwise errors (anchored_length, telo_length) against the planted differences within each planted end."""
    import os
    from topsicle_amd import anchor
    _reads, truth, _tails, telo = ec.detection_reads(ident)
    e_rows = _rows(os.path.join(outdir, f"end_reads_{k}.csv"))[1:]
    a_rows = _rows(os.path.join(outdir, f"anchored_reads_{k}.csv"))
    assert a_rows[0] == anchor.READ_HEADER == ["file", "readID", "tail", "telo_length", "end", "reference", "offset", "votes", "second", "shift", "anchored_length"]
    a_rows = a_rows[1:]
    assert [r[:4] + [r[4]] for r in a_rows] == [r[:4] + [r[7]] for r in e_rows]            # the same reads in the same order, the same groups
    group_of = {r[1]: r[4] for r in a_rows}
    by_group = {}
    for r in a_rows:
        if r[4] == "0":
            assert r[5:] == [""] * 6
            continue
        assert group_of[r[5]] == r[4]                                                       # the reference is a member
        by_group.setdefault(int(r[4]), []).append(r)
        if r[10] != "":
            assert int(r[7]) >= MIN_VOTES and int(r[7]) >= RATIO * int(r[8]) and int(r[10]) == int(r[3]) + int(r[9])
        else:
            assert r[6:] == [""] * 5
    g_rows = _rows(os.path.join(outdir, f"anchored_ends_{k}.csv"))
    assert g_rows[0] == anchor.GROUP_HEADER == ["end", "reads", "anchored", "reference", "consensus_boundary", "anchored_min", "anchored_median", "anchored_mean",
                                                "anchored_max", "called_sd", "anchored_sd"]
    assert [int(r[0]) for r in g_rows[1:]] == sorted(by_group)
    begin = {r[1]: int(r[4]) for r in e_rows}
    for row in g_rows[1:]:
        mem = by_group[int(row[0])]
        anc = [r for r in mem if r[10] != ""]
        assert int(row[1]) == len(mem) and int(row[2]) == len(anc) and {r[5] for r in mem} == {row[3]}
        a = np.array([int(r[10]) for r in anc], np.float64)
        called = np.array([int(r[3]) for r in anc], np.float64)
        assert (int(row[5]), row[6], row[7], int(row[8])) == (int(a.min()), "%.1f" % np.median(a), "%.1f" % a.mean(), int(a.max()))
        assert (row[9], row[10]) == ("%.1f" % np.std(called, ddof=1), "%.1f" % np.std(a, ddof=1))
        # the consensus: the lower median of the members' boundaries in the reference's coordinates; a shift leads there
        pos = sorted(int(r[6]) + begin[row[3]] for r in anc)
        assert int(row[4]) == pos[(len(pos) - 1) // 2]
        assert all(int(r[9]) == int(row[4]) - (int(r[6]) + begin[row[3]]) for r in anc)
    anchored_err, called_err = [], []
    for e in range(1, ec.N_ENDS + 1):
        mine = [r for r in a_rows if truth[int(r[1][4:])] == e and r[10] != ""]
        planted = [telo[int(r[1][4:])] for r in mine]
        anchored_err += orc.pair_errors([int(r[10]) for r in mine], planted)
        called_err += orc.pair_errors([int(r[3]) for r in mine], planted)
    n_anchored = sum(r[10] != "" for r in a_rows)
    return sorted(anchored_err), sorted(called_err), n_anchored
