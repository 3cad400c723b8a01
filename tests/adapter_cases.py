"""The cases the adapter search is checked on (tps_batch_adapter_find; tests/test_adapter.py on the emulation, tests/test_gpu_adapter.py on
the GPU), the oracle's answers for them (tests/adapter_oracle.py, computed once per case and shared), the planted sets of the
detection claim, and a plain-list restatement of the naming rule of topsicle_amd.adapters."""
import functools
import math

import numpy as np

import adapter_oracle as orc
from ends_cases import mutate, rand, repeats, stored_revcomp, write_fasta
from topsicle_amd import synth

ALBICANS23 = "ACGGATGTCTAACTTCTTGGTGT"


class Case:
    def __init__(self, name, patterns):
        self.name, self.patterns = name, list(patterns)
        self.reads, self.tails, self.begin, self.end = [], [], [], []
        self.pairs = []                            # (i, j): rows that must be equal
        self.want = {}                             # read index -> {pattern index: (dist, end)}: answers known by construction
        self.twins = None                          # (j, j'): identical patterns in two lanes

    def add(self, molecule, tail=0, begin=0, end=1024):
        """`molecule` is telomere first; tail 1 stores its reverse complement.  Returns the read's index."""
        self.reads.append(stored_revcomp(molecule) if tail else molecule)
        self.tails.append(tail)
        self.begin.append(begin)
        self.end.append(end)
        return len(self.reads) - 1

    def both(self, molecule, begin=0, end=1024):
        """The molecule on either tail: rows i and i + 1 must be equal."""
        i = self.add(molecule, 0, begin, end)
        self.add(molecule, 1, begin, end)
        self.pairs.append((i, i + 1))
        return i


def _case(name, patterns):
    return Case(name, patterns)


def _lengths():
    """Patterns of 12, 31, 32, 33, 63 and 64 letters, each planted exactly, with ONT errors, and not at all."""
    rng = np.random.default_rng(101)
    pats = [rand(rng, m) for m in (12, 31, 32, 33, 63, 64)]
    c = _case("lengths", pats)
    for j, p in enumerate(pats):
        junk = rand(rng, 5 + 3 * j)
        i = c.both(junk + p + rand(rng, 300), 0, 256)
        c.want[i] = {j: (0, len(junk) + len(p))}
        c.both(rand(rng, 7) + mutate(rng, p, synth.ONT) + repeats("CCCTAA", 400), 0, 256)
        c.both(mutate(rng, rand(rng, 11) + p, (0.08, 0.04, 0.04)) + rand(rng, 100), 0, 256)
    c.both(rand(rng, 1500), 0, 1024)
    return c


def _a64():
    """A x 64 against runs of A: the carry of (Eq & Pv) + Pv crosses bit 31 and reaches bit 63."""
    rng = np.random.default_rng(102)
    c = _case("A64", ["A" * 64])
    for run, want in ((200, (0, 64)), (64, (0, 64)), (63, (1, 63)), (33, (31, 33)), (32, (32, 32)), (31, (33, 31)), (1, (63, 1))):
        i = c.both("A" * run + "C" * 40, 0, 256)
        c.want[i] = {0: want}
    i = c.both("C" * 10 + "A" * 70 + "C" * 40)
    c.want[i] = {0: (0, 74)}
    i = c.both("A" * 30 + "C" + "A" * 33 + "G" * 20)        # one substitution inside 64 letters
    c.want[i] = {0: (1, 64)}
    c.both("A" * 40 + "N" + "A" * 40)
    c.both(mutate(rng, "A" * 300, synth.ONT))
    c2 = ["A" * 63 + "C", "C" + "A" * 63, "A" * 32 + "C" * 32, "AC" * 32]
    d = _case("A64_kin", c2)
    for t in ("A" * 200, "A" * 63 + "C" + "A" * 63, "AC" * 100, "A" * 32 + "C" * 32 + "A" * 32, "C" * 32 + "A" * 32):
        d.both(t + "G" * 17)
    return [c, d]


def _halves():
    """A pattern whose first 32 letters occur in the text but not its last 32, and the other way round."""
    rng = np.random.default_rng(103)
    a, b, x, y = (rand(rng, 32) for _ in range(4))
    c = _case("halves", [a + b, x + y, a + y])
    c.both(rand(rng, 20) + a + rand(rng, 100))               # first half of pattern 0 only
    c.both(rand(rng, 20) + y + rand(rng, 100))               # last half of pattern 1 only
    i = c.both(rand(rng, 20) + a + y + rand(rng, 100))       # pattern 2 whole
    c.want[i] = {2: (0, 84)}
    c.both(rand(rng, 9) + a[:31] + b + rand(rng, 50))        # a deletion at the dword's edge
    c.both(rand(rng, 9) + a + "T" + b + rand(rng, 50))       # an insertion there
    return c


def _counts():
    """P = 1, 2, 63, 64; two identical patterns in different lanes; a list of mixed lengths."""
    rng = np.random.default_rng(104)
    out = []
    for P in (1, 2, 63, 64):
        pats = [rand(rng, int(m)) for m in rng.integers(12, 65, P)]
        if P >= 2:
            pats[-1] = pats[0]                     # lanes 0 and P - 1: identical rows
        c = _case(f"P{P}", pats)
        for r in range(6):
            p = pats[int(rng.integers(0, P))]
            c.add(rand(rng, int(rng.integers(0, 30))) + mutate(rng, p, synth.ONT) + rand(rng, 200), r & 1, 0, 256)
        c.add(rand(rng, 300), 0, 0, 256)
        c.twins = (0, P - 1) if P >= 2 else None
        out.append(c)
    return out


def _regions():
    """n = 0, 1, m - 1, m, 255, 256, 257, 1024; begin at every residue mod 16, past the read; end clamped to L; the empty read."""
    rng = np.random.default_rng(105)
    p = rand(rng, 24)
    m = len(p)
    pats = [p, rand(rng, 40)]
    text = rand(rng, 30) + p + rand(rng, 200) + mutate(rng, p, synth.ONT) + rand(rng, 1500)
    cn = _case("regions_n", pats)
    for n in (0, 1, m - 1, m, 255, 256, 257, 1024):
        cn.both(text, 0, n)
        cn.both(text, 30, 30 + n)                    # (from the occurrence's first letter on)
    cb = _case("regions_begin", pats)
    for b in range(16):
        cb.add(text, b & 1, b, b + 100)
        cb.add(text, (b + 1) & 1, 16 + b, 16 + b + 38)      # the occurrence is [30, 54): whole for b <= 14, its first letter cut for b = 15
    c = _case("regions_edges", pats)
    c.both(text, len(text), len(text) + 100)         # begin at the read's end
    c.both(text, len(text) + 500, len(text) + 600)   # ... past it
    c.both(text, len(text) - 50, len(text) + 900)    # end clamped to L
    c.both(text[:40], 0, 1024)                       # a read shorter than the occurrence's end
    c.both("", 0, 100)                               # the empty read
    c.both("A", 0, 100)
    for L in (63, 64, 65, 127, 128, 129):            # reads that end at, before and behind a quad's edge
        c.add(text[:L], L & 1, 0, 1024)
        c.add(text[:L], (L + 1) & 1, L - 20, L + 20)
    return [cn, cb, c]


def _occurrences():
    rng = np.random.default_rng(106)
    p = rand(rng, 30)
    c = _case("occurrences", [p])
    rest = repeats("CCCTAA", 200)
    i = c.both(p[3:] + rest, 0, 100)                 # at the very start, its first 3 letters missing
    c.want[i] = {0: (3, 27)}
    junk = rand(rng, 50)
    i = c.both(junk + p + rest, 0, 80)               # ends exactly at the region's end
    c.want[i] = {0: (0, 80)}
    c.both(junk + p + rest, 0, 79)                   # cut by the region's end: one letter
    c.both(junk + p + rest, 0, 65)                   # ... half of it
    i = c.both(junk + p + rest, 10, 80)
    c.want[i] = {0: (0, 70)}
    # the same occurrence with other letters outside the region: the same answer
    i = c.both(rand(rng, 10) + junk[10:] + p + rand(rng, 200), 10, 80)
    c.pairs.append((i - 2, i))
    i = c.both("N" * 10 + junk[10:] + p + "N" * 200, 10, 80)
    c.pairs.append((i - 4, i))
    return c


def _ties():
    rng = np.random.default_rng(107)
    p = rand(rng, 19) + "A"                          # ends in ...A
    while p[-2] == "A":
        p = rand(rng, 19) + "A"
    q = p[:9] + ("C" if p[9] != "C" else "G") + p[10:]      # one substitution
    c = _case("ties", [p])
    g1, g2, g3 = rand(rng, 13), rand(rng, 21), rand(rng, 40)
    i = c.both(g1 + p + g2 + p + g3, 0, 256)         # two exact occurrences: the first
    c.want[i] = {0: (0, 33)}
    i = c.both(g1 + q + g2 + q + g3, 0, 256)         # two at distance 1: the first
    c.want[i] = {0: (1, 33)}
    i = c.both(g1 + p + "A" + g2, 0, 256)            # ...A on ...AA: the smaller e
    c.want[i] = {0: (0, 33)}
    i = c.both(g1 + p + g2 + q + g3, 0, 256)         # exact, then one edit
    c.want[i] = {0: (0, 33)}
    i = c.both(g1 + q + g2 + p + g3, 0, 256)         # one edit, then exact
    c.want[i] = {0: (0, 13 + 20 + 21 + 20)}
    return c


def _letters():
    rng = np.random.default_rng(108)
    p = rand(rng, 28)
    c = _case("letters", [p, rand(rng, 16)])
    junk = rand(rng, 17)
    i = c.both(junk + p[:11] + "N" + p[12:] + rand(rng, 100), 0, 256)      # an N inside an occurrence costs 1
    c.want[i] = {0: (1, 45)}
    i = c.both("N" * 300, 0, 256)                    # an all-N region
    c.want[i] = {0: (28, 0), 1: (16, 0)}
    i = c.both((junk + p + rand(rng, 100)).lower(), 0, 256)                # lower case
    c.want[i] = {0: (0, 45)}
    c.both(junk + p[:5] + "RYKM" + p[9:] + "n" * 10 + rand(rng, 50), 0, 256)
    c.both("".join(ch.lower() if k % 3 == 0 else ch for k, ch in enumerate(junk + p + rand(rng, 80))), 3, 200)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    return tuple([_lengths()] + _a64() + [_halves()] + _counts() + _regions() + [_occurrences(), _ties(), _letters()])


def case(name):
    return next(c for c in cases() if c.name == name)


def names():
    return [c.name for c in cases()]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(dist, end) uint16[n, P] of the oracle, computed once per case."""
    c = case(name)
    dist, end = orc.adapter_find(c.reads, c.patterns, c.tails, c.begin, c.end)
    P = len(c.patterns)
    dist, end = np.array(dist, np.uint16).reshape(len(c.reads), P), np.array(end, np.uint16).reshape(len(c.reads), P)
    dist.setflags(write=False)
    end.setflags(write=False)
    return dist, end


def assert_equal(got, name):
    """Bit for bit the oracle's rows."""
    want = expected(name)
    for g, w, what in zip(got, want, ("dist", "end")):
        g = np.asarray(g)
        assert g.dtype == np.uint16 and g.shape == w.shape, (name, what, g.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), f"{name}: {what} of read {bad[0][0]}, pattern {bad[0][1]}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"


def check_oracle(name):
    """What a case knows by construction holds for the oracle's answers (every engine equals the oracle)."""
    c = case(name)
    dist, end = expected(name)
    for i, j in c.pairs:
        assert np.array_equal(dist[i], dist[j]) and np.array_equal(end[i], end[j]), (name, i, j)
    for i, by_pat in c.want.items():
        for j, (d, e) in by_pat.items():
            assert (int(dist[i, j]), int(end[i, j])) == (d, e), (name, i, j, int(dist[i, j]), int(end[i, j]), d, e)
    tw = getattr(c, "twins", None)
    if tw:
        assert np.array_equal(dist[:, tw[0]], dist[:, tw[1]]) and np.array_equal(end[:, tw[0]], end[:, tw[1]])
    if name.startswith("P"):
        assert (dist.min(axis=1)[:6] <= 8).all()   # (the planted pattern is found)


# ---- the refusals of tps_batch_adapter_find: (what differs from a good call, the code in the error message)
REFUSALS = [
    (dict(n_pat=0), "rc=-5"), (dict(n_pat=65), "rc=-5"), (dict(pat_len=11), "rc=-5"), (dict(pat_len=65), "rc=-5"), (dict(end=1025), "rc=-5"),
    (dict(code=(1 << 24, 0)), "rc=-3"), (dict(code=(0, 1), pat_len=32), "rc=-3"), (dict(tail=2), "rc=-3"), (dict(begin=-1), "rc=-3"),
    (dict(begin=5, end=4), "rc=-3"), (dict(n_reads=2), "rc=-3"), (dict(hits_len=1), "rc=-3"),
]


# ---- the naming rule, restated on plain lists
def name_rule(dist_row, lens, err, margin):
    """(best, runner or -1, named) for one read."""
    slack = [int(math.floor(err * m + 1e-9)) - d for d, m in zip(dist_row, lens)]
    best = max(range(len(slack)), key=lambda j: (slack[j], -j))
    if len(slack) == 1:
        return best, -1, slack[best] >= 0
    runner = max((j for j in range(len(slack)) if j != best), key=lambda j: (slack[j], -j))
    return best, runner, slack[best] >= 0 and slack[best] - slack[runner] >= margin


# ---- the detection claim: planted sets
N_DETECT = 240
SETS = {        # name: (P, m, motif, error rates, seed)
    "P1_m28_CCCTAA_ONT": (1, 28, "CCCTAA", synth.ONT, 7101),
    "P12_m24_CCCTAA_ONT": (12, 24, "CCCTAA", synth.ONT, 7102),
    "P4_m40_AAACCCT_ONT": (4, 40, "AAACCCT", synth.ONT, 7103),
    "P24_m24_albicans23_ONT": (24, 24, ALBICANS23, synth.ONT, 7104),
    "P24_m24_albicans23_HIFI": (24, 24, ALBICANS23, synth.HIFI, 7105),
}


@functools.lru_cache(maxsize=None)
def detection_set(ident, n=N_DETECT, tail_len=1500, t_range=(300, 2001)):
    """(patterns, reads, tails, planted pattern or -1, planted end): in three reads of every four mutate(junk + adapter) sits in front
    of mutate(repeats(motif, t) + random bases), junk of 0 .. 40 bases (0 .. 100 for 40-letter adapters), the adapter drawn from the
    set's P random patterns, either tail; the fourth read of every four has no adapter.  The planted end is the length of the
    mutated junk + adapter."""
    P, m, motif, errors, seed = SETS[ident]
    rng = np.random.default_rng(seed)
    pats = [rand(rng, m) for _ in range(P)]
    reads, tails, planted, ends = [], [], [], []
    for i in range(n):
        t = int(rng.integers(*t_range))
        body = mutate(rng, repeats(motif, t, int(rng.integers(0, len(motif)))) + rand(rng, tail_len), errors)
        j, head = -1, ""
        if i % 4 != 3:
            j = int(rng.integers(0, P))
            head = mutate(rng, rand(rng, int(rng.integers(0, 101 if m == 40 else 41))) + pats[j], errors)
        tail = int(rng.integers(0, 2))
        mol = head + body
        reads.append(stored_revcomp(mol) if tail else mol)
        tails.append(tail)
        planted.append(j)
        ends.append(len(head))
    return tuple(pats), tuple(reads), tuple(tails), tuple(planted), tuple(ends)


DETECT_SEARCH = 256


@functools.lru_cache(maxsize=None)
def detection_expected(ident):
    """(dist, end) uint16[n, P] of the oracle's recurrence (adapter_oracle.find_block) for the region [0, 256) of every read of the set,
    computed once."""
    pats, reads, tails, _planted, _ends = detection_set(ident)
    dist, end = orc.find_block(list(pats), [orc.telomere_first(s, t)[:DETECT_SEARCH] for s, t in zip(reads, tails)])
    dist, end = dist.astype(np.uint16), end.astype(np.uint16)
    dist.setflags(write=False)
    end.setflags(write=False)
    return dist, end


def check_detection(dist, end, ident, err=0.2, margin=2):
    """The four conditions of the detection claim on (dist, end) rows for detection_set(ident); returns (named planted reads, planted
    reads, the largest |adapter_end - planted end|)."""
    from topsicle_amd import adapters
    pats, _reads, _tails, planted, ends = detection_set(ident)
    best, _runner, named = adapters.name_reads(dist, [len(p) for p in pats], err, margin)
    n_planted = sum(1 for j in planted if j >= 0)
    good = wrong = false = 0
    worst = 0
    for i, j in enumerate(planted):
        if not named[i]:
            continue
        if j < 0:
            false += 1
        elif int(best[i]) != j:
            wrong += 1
        else:
            good += 1
            worst = max(worst, abs(int(np.asarray(end)[i][int(best[i])]) - ends[i]))
    print(f"{ident}: {good} of {n_planted} planted reads named, {wrong} to a wrong pattern, {false} adapter-free reads named, end error <= {worst}")
    assert good >= 0.97 * n_planted, (ident, good, n_planted)
    assert wrong == 0 and false == 0, (ident, wrong, false)
    assert worst <= 4, (ident, worst)
    return good, n_planted, worst


# ---- `--adapters` end to end: what the CLI tests (host emulation and GPU) run and check
CLI_IDENT, CLI_READS = "P12_m24_CCCTAA_ONT", 48


def write_cli_inputs(tmp_path):
    """(input directory, adapter FASTA): the first 48 reads of the planted set in one file, its 12 patterns named bc01 .. bc12."""
    pats, reads, _tails, _planted, _ends = detection_set(CLI_IDENT, CLI_READS)
    d = tmp_path / "in"
    d.mkdir()
    write_fasta(str(d / "reads.fasta"), reads)
    fa = tmp_path / "adapters.fa"
    fa.write_text("".join(f">bc{j + 1:02d}\n{p}\n" for j, p in enumerate(pats)))
    return str(d), str(fa)


def check_cli_outputs(outdir, k=4):
    """adapters_{k}.csv and adapter_summary_{k}.csv say what the planted set asks for: the headers, one row per read of
    telolengths_all.csv with a stored boundary in that order, the arithmetic of length_from_adapter, the planted pattern where a read
    is named and no adapter-free read named, the summary the sum of the per-read rows.  Returns (rows, named rows)."""
    import csv
    import os
    from topsicle_amd import adapters
    pats, _reads, tails, planted, ends = detection_set(CLI_IDENT, CLI_READS)
    telo = [r for r in csv.DictReader(open(os.path.join(outdir, "telolengths_all.csv"))) if int(r["phrase"]) == k and float(r["telo_length"]) != 0]
    rows = list(csv.reader(open(os.path.join(outdir, f"adapters_{k}.csv"))))
    assert rows[0] == adapters.READ_HEADER
    rows = [dict(zip(rows[0], r)) for r in rows[1:]]
    assert [r["readID"] for r in rows] == [r["readID"] for r in telo]
    named = 0
    for r, t in zip(rows, telo):
        i = int(r["readID"][4:])
        assert r["file"] == "reads" and r["tail"] == ("forward", "reverse")[tails[i]] and int(r["telo_length"]) == int(float(t["telo_length"]))
        assert r["runner"] != "" and r["runner"] != r["adapter"] and int(r["runner_dist"]) >= 0
        if r["adapter"] == "":
            assert r["length_from_adapter"] == ""
            continue
        named += 1
        assert planted[i] >= 0 and r["adapter"] == f"bc{planted[i] + 1:02d}" and int(r["dist"]) <= 4 and abs(int(r["adapter_end"]) - ends[i]) <= 4
        if int(r["adapter_end"]) <= int(r["telo_length"]):
            assert int(r["length_from_adapter"]) == int(r["telo_length"]) - int(r["adapter_end"])
        else:
            assert r["length_from_adapter"] == ""
    summ = list(csv.reader(open(os.path.join(outdir, f"adapter_summary_{k}.csv"))))
    assert summ[0] == adapters.SUMMARY_HEADER
    summ = [dict(zip(summ[0], r)) for r in summ[1:]]
    assert [s["name"] for s in summ] == [f"bc{j + 1:02d}" for j in range(len(pats))] + ["none"]
    for s in summ:
        mine = [r for r in rows if (r["adapter"] or "none") == s["name"]]
        assert int(s["reads"]) == len(mine) and int(s["tail0"]) == sum(r["tail"] == "forward" for r in mine) and int(s["tail1"]) == sum(r["tail"] == "reverse" for r in mine)
        assert s["length"] == ("" if s["name"] == "none" else "24")
        if mine:
            med = lambda xs: sorted(xs)[len(xs) // 2] if len(xs) % 2 else (sorted(xs)[len(xs) // 2 - 1] + sorted(xs)[len(xs) // 2]) / 2      # noqa: E731
            assert float(s["telo_median"]) == med([int(r["telo_length"]) for r in mine])
            if s["name"] != "none":
                assert float(s["dist_median"]) == med([int(r["dist"]) for r in mine]) and float(s["adapter_end_median"]) == med([int(r["adapter_end"]) for r in mine])
                frm = [int(r["length_from_adapter"]) for r in mine if r["length_from_adapter"] != ""]
                assert (s["from_adapter_median"] == "") if not frm else float(s["from_adapter_median"]) == med(frm)
    assert sum(int(s["reads"]) for s in summ) == len(rows)
    return len(rows), named
