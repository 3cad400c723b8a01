"""Test helper: the reads and parameter sets of the boundary refinement tests (tests/test_refine.py on the host emulation,
tests/test_gpu_refine.py on the GPU), and the oracle's answers to them, computed once per process (tests/refine_oracle.py).

Most cases are built by construction: a telomere-first string of exact repeats, in which every position is a hit, with DIPS -- runs of
positions turned into misses by N letters (an isolated N costs exactly the w positions whose word holds it; N letters w apart give a run
of any length >= w) -- and a region that ends where the case needs it.  P is then known position by position, and every builder
asserts, on the oracle's hits, that the case says what it is meant to say."""
import functools
import itertools

import numpy as np

import refine_oracle as orc
import tract_cases

UNITS = {k: tract_cases.UNITS[k] for k in ("CCCTAA", "CCCTAAA", "AAAC", "albicans23", "m32")}
UNITS["AAACCCT"] = UNITS.pop("CCCTAAA")[4:] + "CCCT"           # the same motif, spelled from another letter
assert UNITS["AAACCCT"] == "AAACCCT" and [len(u) for u in UNITS.values()] == [6, 4, 23, 32, 7]
MAX_REGION = 65536
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def piece():
    """Positions of a staged piece: the kernel's own figure."""
    import emu_refine_driver
    return emu_refine_driver.piece()


def revcomp(h):
    """... of a string that may hold N and lower case (the case is kept, another letter stays itself)."""
    comp = dict(_COMP, **{k.lower(): v.lower() for k, v in _COMP.items()})
    return "".join(comp.get(c, c) for c in reversed(h))


def repeats(unit, n, phase=0):
    return tract_cases.repeats(unit, n, phase)


def with_dips(unit, n, dips, letter="N"):
    """n letters of exact repeats in which the positions [start, start + a) of every (start, a) of `dips` are misses (a >= w)."""
    w = min(len(unit), 8)
    h = list(repeats(unit, n, 1))
    for start, a in dips:
        assert a >= w
        for q in list(range(start + w - 1, start + a - 1, w)) + [start + a - 1]:
            h[q] = letter
    return "".join(h)


def prefix(x, hit, miss):
    return [0] + list(itertools.accumulate(hit if v else -miss for v in x))


class Case:
    def __init__(self, name, unit, hit=2, miss=1, sep=200):
        self.name, self.unit, self.hit, self.miss, self.sep = name, unit, hit, miss, sep
        self.reads, self.tails, self.begin, self.end, self.at = [], [], [], [], []

    def add(self, h, tail=0, begin=0, end=None, at=0):
        """The telomere-first string h as a read of `tail`; returns the read's index."""
        self.reads.append(h if tail == 0 else revcomp(h))
        self.tails.append(tail)
        self.begin.append(begin)
        self.end.append(len(h) if end is None else end)
        self.at.append(at)
        return len(self.reads) - 1

    def args(self):
        return self.reads, self.unit, self.tails, self.begin, self.end, self.at

    def kw(self):
        return dict(hit=self.hit, miss=self.miss, sep=self.sep)

    def row(self, i):
        return orc.refine_read(self.reads[i], self.unit, self.tails[i], self.begin[i], self.end[i], self.at[i], **self.kw())

    def P(self, i):
        x = orc.hits(orc.telomere_first(self.reads[i], self.tails[i]), self.unit, self.begin[i], self.end[i])
        return prefix(x, self.hit, self.miss)

    def add_dips(self, n_pos, dips, tail=0, begin=0, at=0, extra=0):
        """A region of n_pos positions from `begin` on, all hits but for `dips` (positions relative to begin); `extra` more letters
        of the read behind the region (end < L), or -1: end lies past the read (end > L)."""
        w = min(len(self.unit), 8)
        n = begin + n_pos + w - 1
        h = with_dips(self.unit, n + max(extra, 0), [(begin + s, a) for s, a in dips])
        i = self.add(h, tail, begin, n + 9 if extra < 0 else n, at)
        x = [1] * n_pos
        for s, a in dips:
            x[s:s + a] = [0] * a
        assert self.P(i) == prefix(x, self.hit, self.miss), (self.name, i)
        return i


def _lengths_case(key):
    """N = 0 (begin = end; a region shorter than a word), 1, 63, 64, 65, a piece +- 1 and two pieces + 1: all hits, so pos is the
    region's end and drop 0.  Both tails, begin 0 and 37, end < L, = L and > L."""
    c = Case(f"lengths_{key}", UNITS[key])
    w = min(len(c.unit), 8)
    pc = piece()
    for n, (tail, begin, extra) in zip((1, 63, 64, 65, pc - 1, pc, pc + 1, 2 * pc + 1, 2, 200, 264),
                                       itertools.cycle([(0, 0, 0), (1, 37, 5), (0, 37, -1), (1, 0, 0), (0, 0, 7), (1, 37, -1)])):
        i = c.add_dips(n, [], tail, begin, at=begin + n // 2, extra=extra)
        r = c.row(i)
        assert r[:3] == (begin + n, c.hit * n, 0) and r[4:6] == (n, 0) and r[3] == c.hit * (n // 2), (key, n, r)
        assert r[6:] == ((c.hit * (n - c.sep), begin + n - c.sep) if n >= c.sep else (0, -1)), (key, n, r)
    for tail, begin, span in ((0, 0, 0), (1, 37, 0), (0, 5, w - 1), (1, 37, 3)):         # N <= 0
        i = c.add(repeats(c.unit, 100), tail, begin, begin + span, at=50)
        assert c.row(i) == (begin, 0, 0, 0, 0, 0, 0, -1)
    i = c.add(repeats(c.unit, 30), 0, 40, 90, at=0)               # begin past the read
    assert c.row(i) == (40, 0, 0, 0, 0, 0, 0, -1)
    c.add("", 0, 0, 0, 0)
    return c


def _no_hits_case():
    """Filler without a single hit: pos = begin, score 0; the runner is the first position sep away."""
    c = Case("no_hits", "CCCTAA")
    for n, tail, begin in ((5, 0, 0), (100, 1, 37), (206, 0, 0), (5000, 1, 37)):
        i = c.add(tract_cases.filler(c.unit, begin + n), tail, begin, at=begin + 3)
        npos = n - 5
        want = (begin, 0, npos, -min(3, npos), 0, 0) if npos > 0 else (begin, 0, 0, 0, 0, 0)
        assert c.row(i)[:6] == want, (n, c.row(i))
        assert c.row(i)[6:] == ((-c.sep, begin + c.sep) if npos >= c.sep else (0, -1))
    return c


def _peak_case(key):
    """The maximum at a given place: the last lane of a step, the first of the next, either side of a piece seam."""
    c = Case(f"peak_{key}", UNITS[key])
    pc = piece()
    for rel, (tail, begin) in zip((1, 63, 64, 65, 128, 129, pc - 1, pc, pc + 1, pc + 64, pc + 65, 2 * pc),
                                  itertools.cycle([(0, 0), (1, 37), (1, 0), (0, 37)])):
        i = c.add_dips(rel + 300, [(rel, 300)], tail, begin, at=begin + rel + 10, extra=11)
        r = c.row(i)
        assert r[:6] == (begin + rel, c.hit * rel, 300 * c.miss, c.hit * rel - 10 * c.miss, rel, 0), (rel, r)
    return c


def _ties_case(hit, miss):
    """Two and three equal maxima: in one lane's positions (64 and 128 apart), in two lanes of one step, in two steps, in two pieces.
    The region ends on the last of them; the smallest wins."""
    c = Case(f"ties_{hit}_{miss}", "CCCTAA", hit, miss)
    pc = piece()
    g = hit + miss
    # a dip of a = u hit misses and b = u miss hits behind it: u (hit + miss) positions further on P is what it was
    def tie(rel, units, tail, begin):
        dips, at_rel = [], rel
        for u in units:
            dips.append((at_rel, u * hit))
            at_rel += u * g
        i = c.add_dips(at_rel, dips, tail, begin, at=begin + at_rel)
        P, r = c.P(i), c.row(i)
        tops = [j for j, v in enumerate(P) if v == max(P)]
        want = [rel] + list(itertools.accumulate((u * g for u in units), initial=rel))[1:]
        assert tops == want and r[0] == begin + rel and r[2] == 0 and r[3] == r[1], (c.name, rel, units, tops, r)
        return tops
    lanes = 64 // g if 64 % g == 0 else None
    if lanes:                                      # (hit + miss divides 64: 1 / 1)
        tie(40, [lanes], 0, 0)                     # one lane, the next step
        tie(40, [lanes, lanes], 1, 37)             # three in one lane
        tie(10, [2 * lanes], 0, 37)                # one lane, two steps on
    tie(10, [6], 0, 0)                             # two lanes of one step
    tie(6, [6, 6], 1, 0)                           # three lanes of one step
    tie(50, [10], 1, 37)                           # two steps
    tie(50, [10, 40], 0, 0)                        # three steps
    tie(pc - 20, [12], 0, 37)                      # either side of a piece seam
    tie(pc - 20, [12, pc // g + 1], 1, 0)          # three pieces
    tie(64, [pc // g], 0, 0)                       # the last lane of step 0 and a later piece
    return c


def _runner_case():
    """The runner on the left and on the right, at distance exactly sep and sep - 1; sep larger than the region; a runner tie
    across a piece seam."""
    c = Case("runner", "CCCTAA", 2, 1, 200)
    pc = piece()
    sep = c.sep
    for d, (tail, begin) in zip((sep, sep - 1, sep + 1), [(0, 0), (1, 37), (0, 37)]):
        # peak A at 300, a dip, peak B (higher) at 300 + d, where the region ends: the runner is on the left
        a = (d // 3) // 2 * 2
        i = c.add_dips(300 + d, [(300, a)], tail, begin)
        P, r = c.P(i), c.row(i)
        assert r[0] == begin + 300 + d and P[300 + d] > P[300] > P[299]
        assert r[6:] == ((P[300], begin + 300) if d >= sep else (P[299], begin + 299)), (d, r)
        # peak A (higher) at 300, a dip, peak B at 300 + d, misses to the end: the runner is on the right
        a = (2 * d // 3) // 2 * 2 + 40
        i = c.add_dips(300 + d + 150, [(300, a), (300 + d, 150)], tail, begin)
        P, r = c.P(i), c.row(i)
        assert r[0] == begin + 300 and P[300] > P[300 + d] > P[100]
        assert r[6:] == ((P[300 + d], begin + 300 + d) if d >= sep else (P[300 + sep], begin + 300 + sep)), (d, r)
    for n in (sep - 1, sep, 150):                  # sep larger than the region; the whole region exactly sep long
        i = c.add_dips(n, [], 0, 0)
        assert c.row(i)[6:] == ((0, 0) if n == sep else (0, -1))
    # two equal peaks either side of the seam, the maximum far behind them at the region's end: the first is the runner
    ja = pc - 30
    i = c.add_dips(ja + 60 + 100 + 200, [(ja, 40), (ja + 60, 100)], 1, 37)
    P, r = c.P(i), c.row(i)
    assert P[ja] == P[ja + 60] and ja < pc < ja + 60 and r[0] == 37 + ja + 360 and r[6:] == (P[ja], 37 + ja), r
    # ... and with the maximum in front of them
    i = c.add_dips(ja + 60 + 300, [(pc - 700, 500), (ja, 40), (ja + 60, 300)], 0, 0)
    P, r = c.P(i), c.row(i)
    assert r[0] == pc - 700 and P[ja] == P[ja + 60] and r[6:] == (P[ja], ja), r
    return c


def _at_case():
    """at = begin, inside, = begin + N, beyond it (clamped), in front of begin (clamped)."""
    c = Case("at", "AAAC")
    for at in (37, 38, 100, 101, 437, 438, 50000, 0, 36):
        i = c.add_dips(400, [(100, 50), (300, 100)], at & 1, 37, at=at)
        P = c.P(i)
        assert c.row(i)[3] == P[min(max(at, 37), 437) - 37]
    return c


def mutate(rng, s, rate):
    out = []
    for ch in s:
        u = rng.random()
        out.append("ACGT"[int(rng.integers(0, 4))] if u < rate else "" if u < 1.2 * rate else ch + "ACGT"[int(rng.integers(0, 4))] if u < 1.4 * rate else ch)
    return "".join(out)


def rand(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def _weights_case(hit, miss):
    """hit / miss at the ends of their range, on noisy tracts of several lengths and on the dips of the other cases."""
    c = Case(f"weights_{hit}_{miss}", "CCCTAA", hit, miss, 100)
    rng = np.random.default_rng(hit)
    pc = piece()
    for n, tail in ((700, 0), (4500, 1), (9000, 0)):
        h = mutate(rng, repeats(c.unit, n // 2), 0.05) + rand(rng, n - n // 2)
        c.add(h, tail, 37 * tail, at=n // 3)
    c.add_dips(pc + 200, [(30, 16), (pc - 8, 16)], 0, 0, at=40)
    c.add_dips(600, [(17, 6), (100, 160), (500, 100)], 1, 37, at=1000)
    return c


def _letters_case(key):
    """N, other letters and lower case, inside and at the edge: an isolated N costs exactly w hits; lower case counts as upper case."""
    c = Case(f"letters_{key}", UNITS[key], sep=50)
    w = min(len(c.unit), 8)
    n = 400
    for q, letter in ((150, "N"), (150, "n"), (150, "R"), (150, "-"), (0, "N"), (n + w - 2, "N"), (w - 1, "N"), (n - 1, "Y")):
        h = list(repeats(c.unit, n + w - 1, 2))
        h[q] = letter
        for tail in (0, 1):
            i = c.add("".join(h), tail, 0, at=q)
            r = c.row(i)
            assert r[4] + r[5] == n - min(w, q + 1, n + w - 1 - q), (key, q, r)
    low = repeats(c.unit, n + w - 1, 2)
    for tail in (0, 1):
        i = c.add(low.lower(), tail, 0, at=7)
        assert c.row(i)[:3] == (n, 2 * n, 0)
        i = c.add(low[:200] + low[200:300].lower() + low[300:], tail, 0, at=7)
        assert c.row(i)[:3] == (n, 2 * n, 0)
    # two N closer than w: fewer than 2 w misses; N at the very edges of a region inside the read
    h = list(repeats(c.unit, 600, 0))
    for q in (37, 37 + 399 + w - 1, 200, 203, 36, 37 + 400 + w - 1):
        h[q] = "N"
    i = c.add("".join(h), 0, 37, 37 + 400 + w - 1, at=0)
    assert sum(c.row(i)[4:6]) == 400 - 1 - 1 - (w + 3)
    c.add("".join(h), 1, 37, 37 + 400 + w - 1, at=0)
    return c


def _full_case():
    """A region of exactly 65 536 letters, either tail: the most steps a read may have."""
    c = Case("full", "CCCTAA")
    rng = np.random.default_rng(9)
    for tail, begin in ((0, 37), (1, 0)):
        h = repeats(c.unit, begin) + mutate(rng, repeats(c.unit, 30000), 0.04)
        h += rand(rng, begin + MAX_REGION - len(h))
        i = c.add(h, tail, begin, at=25000)
        assert c.end[i] - begin == MAX_REGION
    c.add(h + "ACGTACGT", 0, 8, 8 + MAX_REGION, at=3)
    return c


def _ragged_case():
    """300 reads of log-normal length 0 .. 60 000, ONT errors, N in 0.2 % of the places, random tails, regions and `at`; 300 is no
    multiple of the waves of a workgroup."""
    c = Case("ragged", "CCCTAA")
    rng = np.random.default_rng(21)
    for read in tract_cases.ragged().reads:
        L = len(read)
        begin = int(rng.choice([0, 37, 100]))
        end = max(begin, int(rng.choice([L, L + 5, L // 2, 20000])))
        c.reads.append(read)
        c.tails.append(int(rng.integers(0, 2)))
        c.begin.append(begin)
        c.end.append(end)
        c.at.append(int(rng.integers(0, L + 10)))
    import emu_refine_driver
    assert len(c.reads) % emu_refine_driver.wpg()
    return c


@functools.lru_cache(maxsize=None)
def cases():
    out = [_lengths_case(k) for k in UNITS]
    out.append(_no_hits_case())
    out += [_peak_case(k) for k in ("CCCTAA", "m32")]
    out += [_ties_case(1, 1), _ties_case(2, 1), _ties_case(1, 3)]
    out.append(_runner_case())
    out.append(_at_case())
    out += [_weights_case(1, 16), _weights_case(16, 1)]
    out += [_letters_case(k) for k in ("CCCTAA", "AAAC", "albicans23")]
    out.append(_full_case())
    out.append(_ragged_case())
    out.append(Case("empty", "CCCTAA"))
    return tuple(out)


def names():
    return [c.name for c in cases()]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    return orc.boundary_refine(*c.args(), **c.kw())


def assert_equal(got, name):
    want = expected(name)
    assert got.dtype == want.dtype and got.shape == want.shape, name
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{name}: rows differ at reads {bad[:5].tolist()}: got {got[bad[0]]}, want {want[bad[0]]}"


# ---- the refusals: (what differs from a good call on one read of 120 letters, the return code and a piece of the message)
REFUSALS = [
    (dict(unit=(0b0110, 3)), "rc=-3", "4..32 letters"), (dict(unit=(0, 33)), "rc=-3", "4..32 letters"),
    (dict(unit="CCACCA"), "rc=-3", "power of a shorter word"), (dict(unit=(1 << 12, 6)), "rc=-3", "codes behind its letters"),
    (dict(begin=[-1]), "rc=-3", "read 0: need 0 <= begin <= end"), (dict(end=[-1], begin=[-2]), "rc=-3", "read 0: need 0 <= begin <= end"),
    (dict(begin=[5], end=[4]), "rc=-3", "read 0: need 0 <= begin <= end"), (dict(at=[-1]), "rc=-3", "read 0: at must not be negative"),
    (dict(tails=[2]), "rc=-3", "read 0: tail must be 0 or 1"),
    (dict(n_reads=2), "rc=-3", "must hold 1 reads"), (dict(n_reads=0), "rc=-3", "must hold 1 reads"), (dict(out_len=2), "rc=-3", "out must hold 1 rows"),
    (dict(hit=0), "rc=-5", "hit and miss must be 1..16"), (dict(hit=17), "rc=-5", "hit and miss must be 1..16"),
    (dict(miss=0), "rc=-5", "hit and miss must be 1..16"), (dict(miss=17), "rc=-5", "hit and miss must be 1..16"),
    (dict(sep=0), "rc=-5", "sep must be 1..65535"), (dict(sep=65536), "rc=-5", "sep must be 1..65535"),
]
# ... and on two reads of 65 600 letters: a region of 65 537 is refused with the read's number, 65 536 is taken
LONG_REFUSAL = (dict(begin=[0, 63], end=[65536, 65600]), "rc=-5", "read 1: end - begin must be at most 65536")


# ---- `--refine` end to end: what the CLI tests (host emulation and GPU) compare
CLI_READS = 60


def cli_reads(n=CLI_READS):
    """(reads, planted tract lengths): the first n of variant_cases.cli_reads() -- 6000-base ONT reads, half of them telomeric."""
    import variant_cases
    from topsicle_amd import synth
    truth = synth.make_reads(200, 6000, "CCCTAA", seed=5, errors=synth.ONT, tract_min=300, tract_max=3000, telomeric_fraction=0.5)[2]
    return variant_cases.cli_reads()[:n], truth["tract"][:n]


def check_cli_outputs(outdir, reads, unit, ks, trimfirst=100, maxlen=20000, hit=2, miss=1, sep=200, minscore=100, mindrop=100, minmargin=50):
    """Every row of refined_{k}.csv equals the oracle applied to that read with the boundary telolengths_all.csv stores for it, there is
    one row per stored boundary, in run order, and refine_summary_{k}.csv counts the classes of those rows.  Returns the rows of the
    first k as dicts."""
    import csv
    import os
    from topsicle_amd import refine
    w = min(len(unit), 8)
    telo = list(csv.DictReader(open(os.path.join(outdir, "telolengths_all.csv"))))
    first = None
    for k in ks:
        stored = {r["readID"]: int(float(r["telo_length"])) for r in telo if int(r["phrase"]) == k and float(r["telo_length"]) != 0}
        rows = list(csv.reader(open(os.path.join(outdir, f"refined_{k}.csv"))))
        assert rows[0] == refine.READ_HEADER
        assert [r[1] for r in rows[1:]] == [r["readID"] for r in telo if int(r["phrase"]) == k and r["readID"] in stored]
        counts = dict.fromkeys(refine.CLASSES, 0)
        for r in rows[1:]:
            seq = reads[int(r[1][4:])]
            tail = {"forward": 0, "reverse": 1}[r[2]]
            boundary = stored[r[1]]
            assert int(r[3]) == boundary
            pos, score, drop, at_score, before, after, runner, runner_pos = orc.refine_read(seq, unit, tail, trimfirst, maxlen, max(trimfirst, boundary - (w - 1)),
                                                                                            hit, miss, sep)
            n_pos = min(len(seq), maxlen) - trimfirst - w + 1
            length = trimfirst if pos == trimfirst else pos + w - 1
            margin = None if runner_pos < 0 else score - runner
            cls = "no_telomere" if score < minscore else "open" if drop < mindrop else "ambiguous" if margin is not None and margin < minmargin else "clean"
            dens = lambda h, n: "" if n <= 0 else "%.3f" % (h / n)      # noqa: E731
            want = [str(length), str(length - boundary), str(score), str(drop), "" if margin is None else str(margin), str(score - at_score),
                    dens(before, pos - trimfirst), dens(after, n_pos - (pos - trimfirst)), cls]
            assert r[4:] == want, (k, r[1], r[4:], want)
            counts[cls] += 1
        srows = list(csv.reader(open(os.path.join(outdir, f"refine_summary_{k}.csv"))))
        assert srows[0] == refine.SUMMARY_HEADER and [(s[0], int(s[1])) for s in srows[1:]] == [(c, counts[c]) for c in refine.CLASSES]
        if first is None:
            first = [dict(zip(rows[0], r)) for r in rows[1:]]
    return first
