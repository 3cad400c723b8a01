"""Test helper: the reads and parameter sets of the tract map tests (tests/test_tract_map.py on the host emulation,
tests/test_gpu_tract.py on the GPU), and the oracle's answers to them, computed once per process (tests/tract_oracle.py).

The cases are built by construction -- blocks of exact repeats ("1") and blocks of a filler without a single hit ("0") laid out on
the block grid -- and every builder asserts, on the oracle's answer, that the case says what it is meant to say.  Words that
straddle the junction of a repeat block and a filler block may hit: a "0" block next to a "1" block holds a few hits, far below the
thresholds used here; where a count has to be exact the builder searches for it."""
import functools

import numpy as np

import tract_oracle
from topsicle_amd import variants

M32 = "ACGGTTCAGTCCATGACTTGCAAGTCTGATCC"           # 32 letters, no shorter period: fills the uint64
UNITS = {
    "AAAC": "AAAC",
    "CCCTAA": "CCCTAA",
    "CCCTAAA": "CCCTAAA",
    "CCCTAAAA": "CCCTAAAA",
    "m9": "CCCTAAACG",
    "glabrata16": "CTGTGGGGTCTGGGTG",              # exactly one 32-bit word of codes
    "albicans23": "ACGGATGTCTAACTTCTTGGTGT",
    "m32": M32,
}
assert [len(u) for u in UNITS.values()] == [4, 6, 7, 8, 9, 16, 23, 32]
DEFAULTS = dict(block=64, min_hits=20, gap=1, min_blocks=2, max_tracts=8)


def repeats(unit, n, phase=0):
    k = (phase + n) // len(unit) + 2
    return (unit * k)[phase:phase + n]


@functools.lru_cache(maxsize=None)
def filler_word(unit):
    """A short word whose repeats hold no hit on either strand of `unit`, whatever the phase."""
    w = min(len(unit), 8)
    words = tract_oracle.word_set(unit) | tract_oracle.word_set(tract_oracle.revcomp(unit))
    for cand in ("AG", "AC", "GT", "CT", "ACGT", "AGCT", "AAGG", "CCTT", "AGGT", "A", "C"):
        s = repeats(cand, 4 * len(cand) + w)
        if all(s[i:i + w] not in words for i in range(len(s) - w + 1)):
            return cand
    raise AssertionError(f"no filler for {unit}")


def filler(unit, n, phase=0):
    return repeats(filler_word(unit), n, phase)


def layout(unit, flags, block, tail=0, strand=0):
    """A read on the block grid: one block of `block` letters per character of `flags` -- "1" exact repeats of the unit (strand 1:
    of its reverse complement), "0" filler -- and `tail` more letters of filler."""
    u = unit if strand == 0 else tract_oracle.revcomp(unit)
    return "".join(repeats(u, block, 1) if f == "1" else filler(unit, block) for f in flags) + filler(unit, tail)


class Case:
    def __init__(self, name, unit, **kw):
        self.name, self.unit = name, unit
        self.kw = dict(DEFAULTS)
        self.kw.update(kw)
        self.reads = []

    def add(self, read):
        self.reads.append(read)
        return len(self.reads) - 1

    def expect_flags(self, flags, strand=0):
        """The last read added has exactly the flagged blocks of `flags` on `strand` (and none on the other)."""
        w = min(len(self.unit), 8)
        read = self.reads[-1].upper()
        for s, u in enumerate((self.unit, tract_oracle.revcomp(self.unit))):
            counts = tract_oracle.block_counts(read, tract_oracle.word_set(u), w, self.kw["block"])
            got = "".join("1" if c >= self.kw["min_hits"] else "0" for c in counts)
            want = flags if s == strand else "0" * len(flags)
            assert got[:len(want)] == want and "1" not in got[len(want):], (self.name, s, got, want)


def _lengths_case(key):
    """Pure repeats of 0, w - 1, w, w + 1, 63 + w (the last position of block 0), 64 + w (the first of block 1), 128 + w - 1 and
    128 + w letters: nb = 0, a last block of one position, end == L.  min_hits = min_blocks = 1: every block is a tract's."""
    unit = UNITS[key]
    w = min(len(unit), 8)
    c = Case(f"lengths_{key}", unit, min_hits=1, min_blocks=1)
    for L in (0, w - 1, w, w + 1, 63 + w, 64 + w - 1, 64 + w, 128 + w - 1, 128 + w):
        c.add(repeats(unit, L, L % len(unit)))
    return c


def _threshold_case(key, block=64, min_hits=20):
    """A block with exactly min_hits - 1 hits beside one with exactly min_hits: a run of repeats inside the block, away from its
    edges, grown letter by letter until the oracle counts what is asked for."""
    unit = UNITS[key]
    w = min(len(unit), 8)
    words = tract_oracle.word_set(unit)
    c = Case(f"threshold_{key}", unit, block=block, min_hits=min_hits, min_blocks=1, gap=0)

    def block_with(n_hits):
        for x in range(w, block - 2 * w):
            for phase in range(len(unit)):
                s = filler(unit, 4) + repeats(unit, x, phase) + filler(unit, block - 4 - x)
                pad = filler(unit, block) + s + filler(unit, block)
                counts = tract_oracle.block_counts(pad, words, w, block)
                if counts[1] == n_hits and counts[0] == 0 and counts[2] == 0:
                    return s
        raise AssertionError(f"no block with {n_hits} hits for {unit}")
    lo, hi = block_with(min_hits - 1), block_with(min_hits)
    c.add(filler(unit, block) + lo + filler(unit, block) + hi + filler(unit, block + 9))
    c.expect_flags("00010")
    c.add(filler(unit, block) + hi + lo + filler(unit, 13))
    c.expect_flags("010")
    return c


def _gaps_cases():
    """Flagged-block strings inside filler, for every gap and min_blocks: unflagged blocks at the sides never belong to a tract, a
    run shorter than min_blocks is dropped."""
    out = []
    for gap in (0, 1, 2):
        for min_blocks in (1, 2, 3):
            c = Case(f"gaps_g{gap}_b{min_blocks}", "CCCTAA", gap=gap, min_blocks=min_blocks)
            for core in ("101", "1001", "1011", "0110", "11"):
                for strand in (0, 1):
                    flags = "00" + core + "000"
                    c.add(layout("CCCTAA", flags, 64, tail=17, strand=strand))
                    c.expect_flags(flags, strand)
            c.add(layout("CCCTAA", "1011", 64))                # the read starts and ends in a tract
            c.expect_flags("1011")
            out.append(c)
    return out


def _seam_case(block, piece, gap):
    """Tracts and gap blocks on, before and after the cut between two staged pieces (`piece` positions, the kernel's own figure:
    block index piece / block is the first of the second piece), a gap with its flagged sides in different pieces, and a tract
    that is open across three pieces."""
    assert piece % block == 0
    nbp = piece // block
    c = Case(f"seam_block{block}_gap{gap}", "CCCTAA", block=block, min_hits=block // 3, gap=gap, min_blocks=2)
    nb = 2 * nbp + 4

    def flags_with(ones):
        return "".join("1" if j in ones else "0" for j in range(nb))
    for ones in ({nbp - 2, nbp - 1}, {nbp, nbp + 1}, {nbp - 1, nbp}, {nbp - 2, nbp}, {nbp - 1, nbp + 1}, {nbp - 3, nbp - 1}, {nbp, nbp + 2},
                 {nbp - 2, nbp - 1, nbp + 1, nbp + 2}, {2 * nbp - 1, 2 * nbp}, {2 * nbp - 1, 2 * nbp + 1}):
        ones = {j for j in ones if j >= 0}
        c.add(layout("CCCTAA", flags_with(ones), block, tail=block // 2 + 5))
        c.expect_flags(flags_with(ones))
    c.add(layout("CCCTAA", flags_with({nbp - 1, nbp + 2}), block, tail=3))                   # two unflagged blocks between, the cut inside them
    c.expect_flags(flags_with({nbp - 1, nbp + 2}))
    whole = set(range(max(nbp - 2, 0), 2 * nbp + 2))                                          # open from piece 1 through piece 2 into piece 3
    c.add(layout("CCCTAA", flags_with(whole), block, tail=11, strand=1))
    c.expect_flags(flags_with(whole), strand=1)
    return c


def _strands_case():
    c = Case("strands", "CCCTAA")
    g, t = tract_oracle.revcomp("CCCTAA"), "CCCTAA"
    c.add(filler(t, 200) + repeats(g, 500) + repeats(t, 400) + filler(t, 300))               # a G tract runs into a C tract
    c.add(repeats(t, 450, 2) + filler(t, 1000) + repeats(g, 380, 3))                         # a C head and a G tail
    c.add(repeats(g, 450, 2) + filler(t, 1000) + repeats(t, 380, 3))                         # ... and the other way round
    return c


def _selfrc_case():
    """A unit that is its own reverse complement: both strands give equal rows."""
    assert tract_oracle.revcomp("AACGTT") == "AACGTT"
    c = Case("selfrc", "AACGTT")
    c.add(filler("AACGTT", 130) + repeats("AACGTT", 400) + filler("AACGTT", 200) + repeats("AACGTT", 300, 4))
    return c


def _letters_case(key):
    """N inside a tract (words over it do not hit: the block's count drops by exactly w per isolated N), other letters, and a read
    in lower case."""
    unit = UNITS[key]
    w = min(len(unit), 8)
    c = Case(f"letters_{key}", unit)
    base = repeats(unit, 64 * 6 + w - 1)
    c.add(base)
    for at in (100, 64, 63, 0, len(base) - 1):
        c.add(base[:at] + "N" + base[at + 1:])
    c.add(base[:100] + "N" + base[101:130] + "R" + base[131:200] + "n" + base[201:])
    c.add(base.lower())
    c.add(base[:200] + base[200:300].lower() + base[300:])
    c.add("N" * 300)
    words = tract_oracle.word_set(unit)
    full = tract_oracle.block_counts(base, words, w, 64)
    one_n = tract_oracle.block_counts(c.reads[1], words, w, 64)
    assert full == [64] * 6 and one_n == [64, 64 - w, 64, 64, 64, 64]
    return c


def _overflow_cases():
    """More tracts than max_tracts on one strand: found is the true number, the stored tracts are the first ones."""
    out = []
    for max_tracts, strand in ((8, 0), (1, 1), (16, 0)):
        c = Case(f"overflow_{max_tracts}", "CCCTAA", max_tracts=max_tracts)
        flags = "1100" * (max_tracts + 2) + "0"
        c.add(layout("CCCTAA", flags, 64, tail=30, strand=strand))
        c.expect_flags(flags, strand)
        c.add(layout("CCCTAA", "1100" * max_tracts, 64, tail=30, strand=strand))             # exactly max_tracts
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def ragged():
    """300 reads of log-normal length, 0 .. 60 000 letters (some shorter than a word), ONT errors, N in 0.2 % of the places; 300
    is no multiple of the waves of a workgroup."""
    from topsicle_amd import synth
    b, o, _ = synth.make_ragged_reads(300, "CCCTAA", seed=11, errors=synth.ONT, len_mu=8.3, len_sigma=1.1, min_len=3, max_len=60000,
                                      n_frac=0.002, tract_min=300, tract_max=6000)
    c = Case("ragged", "CCCTAA")
    c.reads = synth.split_reads(b, o)
    for i, n in ((5, 0), (100, 3), (171, 5), (299, 6)):         # (the generator's shortest read is longer than a word)
        c.reads[i] = c.reads[i][:n]
    lens = [len(r) for r in c.reads]
    assert min(lens) < 6 and max(lens) > 30000 and len(lens) % 8
    return c


def _long_case():
    """One read of 200 000 letters with eight scattered tracts, on both strands."""
    rng = np.random.default_rng(3)
    unit = "CCCTAA"
    parts, at = [], 0
    starts = [1000, 20011, 45000, 70123, 100000, 130500, 160064, 199000]
    for i, s in enumerate(starts):
        parts.append(filler(unit, s - at))
        n = int(rng.integers(300, 900)) if i < 7 else 1000
        parts.append(repeats(unit if i % 2 == 0 else tract_oracle.revcomp(unit), n, i))
        at = s + n
    c = Case("long", unit)
    c.add("".join(parts))
    assert len(c.reads[0]) == 200000
    return c


@functools.lru_cache(maxsize=None)
def cases():
    import emu_tract_driver
    out = [_lengths_case(k) for k in UNITS]
    out += [_threshold_case("CCCTAA"), _threshold_case("albicans23"), _threshold_case("AAAC", min_hits=12)]
    out += _gaps_cases()
    out += [_seam_case(b, emu_tract_driver.piece(b), gap) for b in (64, 128, 1024) for gap in (1, 2)]
    out += [_strands_case(), _selfrc_case()]
    out += [_letters_case(k) for k in ("CCCTAA", "glabrata16")]
    out += _overflow_cases()
    out += [ragged(), _long_case(), Case("empty", "CCCTAA")]
    return tuple(out)


CASE_IDS = [c.name for c in cases()]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(tracts, found, totals) of the oracle for case `name`."""
    c = case(name)
    return tract_oracle.tract_map(c.reads, c.unit, **c.kw)


def assert_equal(got, name):
    want = expected(name)
    for what, g, w in zip(("tracts", "found", "totals"), got, want):
        assert g.shape == w.shape, (name, what, g.shape, w.shape)
        if what == "tracts":
            for f in ("begin", "end", "hits", "blocks"):
                bad = np.argwhere(g[f] != w[f])
                assert len(bad) == 0, f"{name}: tracts.{f} differs at (read, strand, tract) {bad[:5].tolist()}: got {g[f][tuple(bad[0])]}, want {w[f][tuple(bad[0])]}"
        else:
            assert g.dtype == w.dtype
            bad = np.argwhere(g != w)
            assert len(bad) == 0, f"{name}: {what} differs at {bad[:5].tolist()}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"


# ---- `--tracts` end to end: what the CLI tests (host emulation and GPU) compare
PLANTED = {"fusion": range(0, 10), "both_ends": range(10, 20), "interstitial": range(20, 30)}


def cli_reads(n=200, read_len=6000):
    """n synthetic reads of read_len bases (ONT errors, half of them telomeric: CCCTAA at the head or TTAGGG at the tail); the
    first 30 are replaced by reads built by construction: 10 fusions (a G tract that runs into a C tract, mid-read), 10 reads
    with a C tract at the head and a G tract at the tail, 10 with one tract in the middle."""
    from topsicle_amd import synth
    b, o, _ = synth.make_reads(n, read_len, "CCCTAA", seed=5, errors=synth.ONT, tract_min=300, tract_max=3000, telomeric_fraction=0.5)
    reads = synth.split_reads(b, o)
    rng = np.random.default_rng(9)
    t, g = "CCCTAA", "TTAGGG"
    rand = lambda k: "".join("ACGT"[j] for j in rng.integers(0, 4, k))      # noqa: E731
    for i in PLANTED["fusion"]:
        a, b_, c = int(rng.integers(1500, 2500)), int(rng.integers(400, 900)), int(rng.integers(400, 900))
        reads[i] = rand(a) + repeats(g, b_, i) + repeats(t, c, i) + rand(read_len - a - b_ - c)
    for i in PLANTED["both_ends"]:
        a, c = int(rng.integers(400, 1200)), int(rng.integers(400, 1200))
        reads[i] = repeats(t, a, i) + rand(read_len - a - c) + repeats(g, c, i)
    for i in PLANTED["interstitial"]:
        a, b_ = int(rng.integers(1500, 3500)), int(rng.integers(400, 900))
        reads[i] = rand(a) + repeats(t if i % 2 else g, b_, i) + rand(read_len - a - b_)
    assert all(len(r) == read_len for r in reads)
    return reads


def write_fasta(path, reads):
    with open(path, "w") as fh:
        fh.write("".join(f">read{i}\n{s}\n" for i, s in enumerate(reads)))


def check_cli_outputs(outdir, reads, unit, edge=256, file_name="reads", **kw):
    """tracts.csv and tract_reads.csv equal what the oracle and tracts.classify give for the same reads.  Returns the classes by
    read index."""
    import csv
    import os
    from topsicle_amd import tracts
    p = dict(DEFAULTS)
    p.update(kw)
    mt = p.pop("max_tracts")
    slack = p["block"] + min(len(unit), 8) - 1          # what the CLI allows two abutting tracts to overlap (tracts.TractSpec.slack)
    want_t, want_r, classes = [], [], {}
    for i, read in enumerate(reads):
        t0, t1, _ = tract_oracle.map_read(read, unit, **p)
        cls = tracts.classify(len(read), [(b, e) for b, e, _h, _n in t0], [(b, e) for b, e, _h, _n in t1], edge, slack)
        classes[i] = cls
        if not t0 and not t1:
            continue
        for strand, ts in (("C", t0), ("G", t1)):
            want_t += [[file_name, f"read{i}", str(len(read)), strand, str(b), str(e), str(nb), str(h)] for b, e, h, nb in ts[:mt]]
        want_r.append([file_name, f"read{i}", str(len(read)), str(len(t0)), str(len(t1)), cls, "1" if max(len(t0), len(t1)) > mt else "0"])
    got_t = list(csv.reader(open(os.path.join(outdir, "tracts.csv"))))
    got_r = list(csv.reader(open(os.path.join(outdir, "tract_reads.csv"))))
    assert got_t[0] == tracts.TRACT_HEADER and got_r[0] == tracts.READ_HEADER
    assert got_t[1:] == want_t
    assert got_r[1:] == want_r
    return classes


# ---- the refusals: (what differs from a good call, the return code in the message)
REFUSALS = [
    (dict(code=variants.unit_code("CCT")[0], m=3), "rc=-3"), (dict(code=0, m=33), "rc=-3"), (dict(code=variants.unit_code("CCACCA")[0]), "rc=-3"),
    (dict(code=variants.unit_code("CCCTAA")[0] | 1 << 12), "rc=-3"),
    (dict(lens=(15, 2, 4)), "rc=-3"), (dict(lens=(16, 3, 4)), "rc=-3"), (dict(lens=(16, 2, 5)), "rc=-3"),
    (dict(block=0), "rc=-5"), (dict(block=96), "rc=-5"), (dict(block=1088), "rc=-5"),
    (dict(min_hits=0), "rc=-5"), (dict(min_hits=65), "rc=-5"), (dict(gap=-1), "rc=-5"), (dict(gap=65), "rc=-5"),
    (dict(min_blocks=0), "rc=-5"), (dict(min_blocks=65), "rc=-5"), (dict(max_tracts=0, lens=(0, 2, 4)), "rc=-5"), (dict(max_tracts=17, lens=(34, 2, 4)), "rc=-5"),
]
