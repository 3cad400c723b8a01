"""Test helper: the reads, tracts and parameter sets of the variant census tests (tests/test_variant_census.py on the host emulation,
tests/test_gpu_variant.py on the GPU), and the oracle's answers to them, computed once per process (tests/variant_oracle.py).

Every read is built as h, the string the rule looks at ("telomere first"), and handed over as h (tail 0) or as its reverse
complement (tail 1).  The kernel walks a tract back from its end in pieces of `bin` positions, so the edges of its staged pieces
are the bin edges: end - bin, end - 2 bin, ... (in the last, clipped bin too)."""
import functools

import numpy as np

import variant_oracle
from topsicle_amd import variants

M32 = "ACGGTTCAGTCCATGACTTGCAAGTCTGATCC"           # 32 letters, no shorter period: fills the uint64
UNITS = {
    "AAAC": "AAAC",                                # x = AAAA is at distance 1 from all four rotations
    "CCCTAA": "CCCTAA",
    "CCCTAAA": "CCCTAAA",
    "CCCTAAAA": "CCCTAAAA",
    "glabrata16": "CTGTGGGGTCTGGGTG",              # exactly one 32-bit word of codes
    "albicans23": "ACGGATGTCTAACTTCTTGGTGT",
    "m32": M32,
}
assert [len(u) for u in UNITS.values()] == [4, 6, 7, 8, 16, 23, 32]
_COMP = str.maketrans("ACGTacgtNn", "TGCAtgcaNn")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def repeats(unit, n, phase=0):
    k = (phase + n) // len(unit) + 2
    return (unit * k)[phase:phase + n]


def noisy(unit, n, rng, sub=0.03, other=0.004):
    """n letters of repeats with substitutions and, rarer, an N or a lower-case letter."""
    s = list(repeats(unit, n, int(rng.integers(0, len(unit)))))
    for i in np.nonzero(rng.random(n) < sub)[0]:
        s[i] = "ACGT"[int(rng.integers(0, 4))]
    for i in np.nonzero(rng.random(n) < other)[0]:
        s[i] = "N" if rng.random() < 0.5 else s[i].lower()
    return "".join(s)


class Case:
    def __init__(self, name, unit, bin=500, n_bins=40):
        self.name, self.unit, self.bin, self.n_bins = name, unit, bin, n_bins
        self.reads, self.tails, self.begin, self.end = [], [], [], []

    def add(self, h, tail, begin, end):
        """h = the oriented string; the tract is [begin, end) of it."""
        self.reads.append(h if tail == 0 else revcomp(h))
        self.tails.append(tail)
        self.begin.append(begin)
        self.end.append(end)

    def args(self):
        return (list(self.reads), self.unit, np.array(self.tails, np.uint8), np.array(self.begin, np.int32), np.array(self.end, np.int32))

    def kw(self):
        return dict(bin=self.bin, n_bins=self.n_bins)


def _lengths_case(key, bin=64, n_bins=3):
    """Tracts of m - 1, m, m + 1 bases; 63, 64, 65 examined positions; a tract and its last position one either side of a bin (=
    staged-piece) edge; tracts longer than bin * n_bins; begin = 0 and begin = 37; end = L, end < L, end > L; both tails; read
    lengths that are odd, no multiple of 16 or 64."""
    unit = UNITS[key]
    m = len(unit)
    rng = np.random.default_rng(100 + m)
    c = Case(f"lengths_{key}" + ("" if n_bins == 3 else f"_bins{n_bins}"), unit, bin, n_bins)
    lens = [m - 1, m, m + 1, 62 + m, 63 + m, 64 + m, bin - 1, bin, bin + 1, bin + m - 2, bin + m - 1, bin + m, 2 * bin - 1, 2 * bin, 2 * bin + 1,
            bin * n_bins - 1, bin * n_bins, bin * n_bins + 1, bin * n_bins + bin + 7, 5 * bin + 3]
    n = 0
    for t in lens:
        for tail in (0, 1):
            for begin in (0, 37):
                extra = (0, 13, 0, 29)[n & 3]
                h = noisy(unit, begin + t + extra, rng)
                # every fourth read asks for more than it has: end > L, clamped to L = begin + t
                end = begin + t + (5 if (n & 3) == 2 else 0)
                c.add(h, tail, begin, end)
                n += 1
    assert any(len(r) % 2 and len(r) % 16 and len(r) % 64 for r in c.reads)
    return c


def _straddle_case(key, bin=64):
    """One substituted unit in exact repeats, at every offset around the first and the second bin edge (the edges of the staged
    pieces) and around the edge of the last, clipped bin's second piece."""
    unit = UNITS[key]
    m = len(unit)
    c = Case(f"straddle_{key}", unit, bin, 2)
    L = 4 * bin + 3 * m + 5
    for tail in (0, 1):
        for edge in (L - bin, L - 2 * bin, L - 3 * bin):
            for d in (-m, -m + 1, -2, -1, 0, 1, m - 1):
                h = list(repeats(unit, L, 1))
                h[edge + d] = "ACGT"[("ACGT".index(h[edge + d]) + 1) % 4]
                c.add("".join(h), tail, 3, L)
    return c


def _letters_case(key):
    """N and lower-case letters inside the tract, at its first and last m-mer, and just outside it."""
    unit = UNITS[key]
    m = len(unit)
    c = Case(f"letters_{key}", unit, 64, 4)
    L, begin, end = 301, 21, 280
    for tail in (0, 1):
        for at in (begin - 1, begin, begin + m - 1, begin + m, 150, end - m - 1, end - m, end - 1, end):
            for what in ("N", "lower", "R"):
                h = list(repeats(unit, L, 2))
                h[at] = h[at].lower() if what == "lower" else what
                c.add("".join(h), tail, begin, end)
        c.add(repeats(unit, L, 2).lower(), tail, begin, end)
        c.add("N" * L, tail, begin, end)
    return c


@functools.lru_cache(maxsize=None)
def ragged():
    """~40 reads of 50 .. 9000 bases, tracts of any length inside them, some reads without one (begin = end = 0)."""
    rng = np.random.default_rng(7)
    c = Case("ragged", "CCCTAA", 500, 40)
    lens = [50, 51, 63, 64, 65, 127, 500, 501, 506, 999, 1000, 1001, 1337, 2048, 4095, 4096, 4097, 8191, 9000] + [int(x) for x in rng.integers(50, 9000, 21)]
    for i, L in enumerate(lens):
        tail = int(rng.integers(0, 2))
        h = noisy("CCCTAA", L, rng)
        if i % 7 == 3:
            c.add(h, tail, 0, 0)
            continue
        begin = int(rng.integers(0, min(L, 120)))
        end = int(rng.integers(begin, L + 1)) if i % 3 else L
        if i % 5 == 0:
            # the subtelomere behind the tract: random letters (mostly "other")
            k = (begin + end) // 2
            h = h[:begin] + h[begin:k] + "".join("ACGT"[j] for j in rng.integers(0, 4, L - k))
        c.add(h, tail, begin, end)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    out = [_lengths_case(k) for k in UNITS]
    out += [_lengths_case("AAAC", n_bins=1), _lengths_case("m32", n_bins=1), _lengths_case("CCCTAAA", bin=100, n_bins=2)]
    out += [_straddle_case(k) for k in ("CCCTAA", "CCCTAAA", "albicans23", "m32")]
    out += [_letters_case(k) for k in ("CCCTAA", "glabrata16", "m32")]
    out.append(ragged())
    rng = np.random.default_rng(5)
    # one 20 000-base tract, either tail: the default bins, and the widest bin (the largest staged piece)
    for key, bin, n_bins in (("CCCTAA", 500, 40), ("m32", 4064, 2), ("albicans23", 4064, 64), ("CCCTAA", 64, 64)):
        c = Case(f"long_{key}_bin{bin}", UNITS[key], bin, n_bins)
        for tail in (0, 1):
            c.add(noisy(UNITS[key], 20131, rng), tail, 100, 20100)
        out.append(c)
    out.append(Case("empty", "CCCTAA"))
    return tuple(out)


CASE_IDS = [c.name for c in cases()]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(counts, profile) of the oracle for case `name`."""
    c = case(name)
    return variant_oracle.variant_census(*c.args(), **c.kw())


def assert_equal(got_counts, got_profile, name, with_profile=True):
    want_counts, want_profile = expected(name)
    assert got_counts.dtype == np.uint32 and got_counts.shape == want_counts.shape
    bad = np.argwhere(got_counts != want_counts)
    assert len(bad) == 0, f"{name}: counts differ at (read, column) {bad[:5].tolist()}: got {got_counts[tuple(bad[0])]}, want {want_counts[tuple(bad[0])]}"
    if with_profile:
        assert got_profile.dtype == np.int64 and got_profile.shape == want_profile.shape
        bad = np.argwhere(got_profile != want_profile)
        assert len(bad) == 0, f"{name}: profile differs at (bin, column) {bad[:5].tolist()}"
    else:
        assert got_profile is None


# ---- the isolated-variant case: its expectation comes from the construction, not from the oracle
ISOLATED = [("CCCTAA", 3, "C", "T4C"), ("CCCTAAA", 5, "G", "A6G"), ("ACGGATGTCTAACTTCTTGGTGT", 22, "A", "T23A")]


def isolated(unit, place, letter, planted=7, tail=0):
    """(read, begin, end): 60 exact units with `planted` units, four units apart and away from the ends, whose letter at `place`
    (0-based) reads `letter`."""
    m = len(unit)
    h = list(unit * 60)
    for k in range(planted):
        h[(5 + 4 * k) * m + place] = letter
    h = "".join(h)
    return (h if tail == 0 else revcomp(h)), 0, len(h)


# ---- `--variants` end to end: what the CLI tests (host emulation and GPU) compare
def cli_reads(n=200):
    """n synthetic 6000-base ONT reads, half of them telomeric (tracts of 300 .. 3000 bases of CCCTAA)."""
    from topsicle_amd import synth
    b, o, _ = synth.make_reads(n, 6000, "CCCTAA", seed=5, errors=synth.ONT, tract_min=300, tract_max=3000, telomeric_fraction=0.5)
    return synth.split_reads(b, o)


def write_fasta(path, reads):
    with open(path, "w") as fh:
        fh.write("".join(f">read{i}\n{s}\n" for i, s in enumerate(reads)))


def check_cli_outputs(outdir, reads, unit, ks, bin=500, n_bins=40, trimfirst=100):
    """Every row of variants_{k}.csv equals the oracle applied to that read with the boundary telolengths_all.csv stores for it, there
    is one row per stored boundary, and variant_profile_{k}.csv is the sum of the oracle's profiles.  Returns the rows checked."""
    import csv
    import os
    from topsicle_amd import variants
    telo = list(csv.DictReader(open(os.path.join(outdir, "telolengths_all.csv"))))
    checked = 0
    for k in ks:
        stored = {r["readID"]: int(float(r["telo_length"])) for r in telo if int(r["phrase"]) == k and float(r["telo_length"]) != 0}
        rows = list(csv.reader(open(os.path.join(outdir, f"variants_{k}.csv"))))
        assert rows[0] == variants.READ_HEADER + variants.class_names(unit)
        assert [r[1] for r in rows[1:]] == [r["readID"] for r in telo if int(r["phrase"]) == k and r["readID"] in stored]
        profile = np.zeros((n_bins, 2 + 4 * len(unit)), np.int64)
        for r in rows[1:]:
            seq = reads[int(r[1][4:])]
            tail = {"forward": 0, "reverse": 1}[r[2]]
            assert (int(r[3]), int(r[4])) == (trimfirst, stored[r[1]])
            row, prof = variant_oracle.census_read(seq, unit, tail, trimfirst, stored[r[1]], bin, n_bins)
            profile += prof
            assert [int(x) for x in r[5:]] == list(variants.split_row(row, unit)[:3]) + variants.split_row(row, unit)[3], r[1]
            checked += 1
        prows = list(csv.reader(open(os.path.join(outdir, f"variant_profile_{k}.csv"))))
        assert prows[0] == variants.PROFILE_HEADER + variants.class_names(unit) and len(prows) == 1 + n_bins
        for b, pr in enumerate(prows[1:]):
            s = variants.split_row(profile[b], unit)
            assert [int(x) for x in pr] == [b * bin] + list(s[:3]) + s[3], (k, b)
    return checked


# ---- the refusals: (what differs from a good call, the return code in the message)
REFUSALS = [
    (dict(code=0b0110, m=1), "rc=-3"), (dict(code=0, m=33), "rc=-3"), (dict(code=variants.unit_code("CCACCA")[0]), "rc=-3"),
    (dict(code=variants.unit_code("AA")[0], m=2), "rc=-3"), (dict(code=1 << 12), "rc=-3"),
    (dict(begin=[-1]), "rc=-3"), (dict(end=[-1], begin=[-2]), "rc=-3"), (dict(begin=[5], end=[4]), "rc=-3"), (dict(tails=[2]), "rc=-3"),
    (dict(tails=[0, 0], begin=[0, 0], end=[1, 1]), "rc=-3"),
    (dict(bin=63), "rc=-5"), (dict(bin=4065), "rc=-5"), (dict(n_bins=0), "rc=-5"), (dict(n_bins=65), "rc=-5"),
]
