"""Test helper: the reads, windows and parameter sets of the end-group tests (tests/test_end_sketch.py on the host emulation,
tests/test_gpu_ends.py on the GPU), the hand-built sketch sets of the link tests, the planted-end detection sets, and the oracle's
answers to all of them, computed once per process (tests/ends_oracle.py)."""
import functools

import numpy as np

import ends_oracle as orc
from topsicle_amd import synth
from topsicle_amd.variants import unit_code
from tract_cases import M32, repeats

UNITS = {"AAAC": "AAAC", "CCCTAA": "CCCTAA", "AAACCCT": "AAACCCT", "albicans23": "ACGGATGTCTAACTTCTTGGTGT", "m32": M32}
assert [len(u) for u in UNITS.values()] == [4, 6, 7, 23, 32]
EMPTY = orc.EMPTY


_STORE = str.maketrans("ACGTacgt", "TGCAtgca")


def stored_revcomp(s):
    """The reverse complement as a file would hold it: case kept, letters that are not ACGT left as they are."""
    return s[::-1].translate(_STORE)


def rand(rng, n):
    return "".join("ACGT"[j] for j in rng.integers(0, 4, n))


def clean_random(rng, n, unit):
    """n random letters without a single repeat word of `unit` (either strand): letter by letter, another letter where one would end
    a repeat word, and the last w letters again where none fits (five letters of a cyclic word take no sixth)."""
    words, w = orc.repeat_words(unit), min(len(unit), 8)
    s = []
    while len(s) < n:
        for c in rng.permutation(4):
            s.append("ACGT"[c])
            if len(s) < w or "".join(s[-w:]) not in words:
                break
            s.pop()
        else:
            del s[-w:]
    return "".join(s)


def mutate(rng, s, errors):
    """`s` with the substitution / insertion / deletion rates of topsicle_amd.synth (ONT, HIFI) applied letter by letter."""
    sub, ins, dele = errors
    r = rng.random((len(s), 3))
    new = rng.integers(0, 4, (len(s), 2))
    out = []
    for i, c in enumerate(s):
        if r[i, 2] < dele:
            continue
        out.append("ACGT"[new[i, 0]] if r[i, 0] < sub else c)
        if r[i, 1] < ins:
            out.append("ACGT"[new[i, 1]])
    return "".join(out)


class Case:
    def __init__(self, name, unit, k=12, buckets=256):
        self.name, self.unit, self.k, self.buckets = name, unit, k, buckets
        self.reads, self.tails, self.begin, self.end = [], [], [], []

    def add(self, molecule, tail, begin, end):
        """`molecule` is telomere first; tail 1 stores its reverse complement."""
        self.reads.append(stored_revcomp(molecule) if tail else molecule)
        self.tails.append(tail)
        self.begin.append(begin)
        self.end.append(end)
        return len(self.reads) - 1

    def add_raw(self, read, tail, begin, end):
        self.reads.append(read)
        self.tails.append(tail)
        self.begin.append(begin)
        self.end.append(end)
        return len(self.reads) - 1


def _mirror_case(key, k=12, buckets=256, name=None):
    """Tail 0 and tail 1 of the same molecules -- 300 bases of telomere, then random subtelomere: equal rows."""
    unit = UNITS[key]
    rng = np.random.default_rng(100 + len(unit) + k + buckets)
    c = Case(name or f"mirror_{key}", unit, k, buckets)
    for i in range(3):
        mol = repeats(unit, 300, i) + rand(rng, 1500 + 37 * i)
        for tail in (0, 1):
            c.add(mol, tail, 280 + i, 1700)
    return c


def _head_case():
    """A window whose first 300 bases are telomere with ONT errors: its k-mers are nearly all left out."""
    rng = np.random.default_rng(11)
    c = Case("telomere_head", "CCCTAA")
    for i in range(4):
        c.add(mutate(rng, repeats("CCCTAA", 320, i), synth.ONT)[:300] + clean_random(rng, 200, "CCCTAA"), i & 1, 0, 500)
    return c


SEAM_K, SEAM_UNIT = 12, "CCCTAA"


def seam_places(piece):
    """Where the seam case puts its exact repeat words (window coordinates): at every place from the last word of piece 0's last
    k-mer to the first letter piece 0 does not stage, at the second cut, and alone in a clean stretch (the last-word test)."""
    return [piece + SEAM_K - 1 - d for d in range(0, SEAM_K)] + [2 * piece - 3], 700


def _seam_case(piece):
    """Windows of more than two pieces in clean random sequence with exact repeat words planted around the cuts: a piece stages
    positions [lo, lo + piece + k - 1), so a word that starts at lo + piece + k - 1 - d, 0 < d < w, straddles the end of what piece 0
    staged.  One word sits alone at `lone`: the k-mers that end with it are dropped, the one before them is kept."""
    rng = np.random.default_rng(12)
    c = Case("seam", SEAM_UNIT, SEAM_K)
    begin = 150
    places, lone = seam_places(piece)
    for n, p in enumerate(places):
        for tail in (n & 1,):
            s = list(clean_random(rng, begin + 2 * piece + 900, SEAM_UNIT))
            for at in (p, lone):
                s[begin + at:begin + at + len(SEAM_UNIT)] = SEAM_UNIT
            c.add("".join(s), tail, begin, begin + 2 * piece + 800)
    return c


def _letters_case():
    """N and other letters, lower case, inside the window; both tails."""
    rng = np.random.default_rng(13)
    c = Case("letters", "CCCTAA")
    base = repeats("CCCTAA", 100) + rand(rng, 900)
    for tail in (0, 1):
        c.add(base, tail, 50, 1000)
        s = list(base)
        for p in (120, 121, 300, 511, 512, 999):
            s[p] = "N"
        s[700] = "R"
        c.add("".join(s), tail, 50, 1000)
        c.add(base.lower(), tail, 50, 1000)
        c.add("".join(ch.lower() if i % 3 else ch for i, ch in enumerate(s)), tail, 50, 1000)
        c.add("N" * 400, tail, 0, 400)
    return c


def _bounds_case(k):
    """end past the read, begin past the read, windows of exactly k - 1 and k letters, empty windows and an empty read."""
    rng = np.random.default_rng(14 + k)
    c = Case(f"bounds_k{k}", "CCCTAA", k)
    mol = clean_random(rng, 600, "CCCTAA")
    for tail in (0, 1):
        c.add(mol, tail, 100, 600 + 500)           # end past the read: clamped
        c.add(mol, tail, 100, 600)
        c.add(mol, tail, 700, 900)                 # begin past the read
        c.add(mol, tail, 200, 200 + k - 1)         # no k-mer
        c.add(mol, tail, 200, 200 + k)             # exactly one
        c.add(mol, tail, 600 - k, 600)             # the read's last k-mer
        c.add(mol, tail, 600 - k + 1, 600 + 9)     # k - 1 letters after the clamp
        c.add(mol, tail, 0, 0)
    c.add_raw("", 0, 0, 0)
    c.add_raw("ACGT", 1, 0, 4)
    return c


def _longest_case():
    """The longest window the call takes (16384), on both tails, and one inside a longer read."""
    rng = np.random.default_rng(15)
    c = Case("longest", "CCCTAA")
    mol = repeats("CCCTAA", 500) + rand(rng, 17000)
    c.add(mol, 0, 400, 400 + 16384)
    c.add(mol, 1, 400, 400 + 16384)
    c.add(mol[:9000], 1, 0, 16384)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    import emu_ends_driver
    out = [_mirror_case(key) for key in UNITS]
    out += [_head_case(), _seam_case(emu_ends_driver.piece()), _letters_case(), _bounds_case(8), _bounds_case(12), _bounds_case(16), _longest_case()]
    out += [_mirror_case("CCCTAA", k, 256, f"k{k}") for k in (8, 16)]
    out += [_mirror_case("AAACCCT", 12, b, f"buckets{b}") for b in (64, 128, 256, 512)]
    out += [_mirror_case("albicans23", 16, 512, "albicans23_k16_b512"), _mirror_case("AAAC", 8, 64, "AAAC_k8_b64"), Case("empty", "CCCTAA")]
    return tuple(out)


CASE_IDS = [c.name for c in cases()]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(sketch, kept) of the oracle for case `name`."""
    c = case(name)
    return orc.end_sketch(c.reads, c.unit, c.tails, c.begin, c.end, c.k, c.buckets)


def assert_equal(got, name):
    want = expected(name)
    for what, g, w in zip(("sketch", "kept"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, what, g.shape, w.shape, g.dtype)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{name}: {what} differs at {bad[:5].tolist()}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"


# ---- links: hand-built sketch sets
def _row(buckets, rng):
    """A row of distinct random hashes (none equal to EMPTY; no two rows of a set share one by chance: 32-bit values)."""
    return rng.integers(0, 0xFFFFFFF0, buckets, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def link_sets():
    """{name: (sketch, min_match, max_links)}"""
    out = {}
    rng = np.random.default_rng(21)
    B = 64
    # ties: rows 1 .. 3 share exactly min_match - 1, min_match, min_match + 1 buckets with row 0; row 4 would share 20, all EMPTY
    s = np.stack([_row(B, rng) for _ in range(6)])
    for j, share in ((1, 5), (2, 6), (3, 7)):
        s[j, :share] = s[0, :share]
    s[0, 40:60] = EMPTY
    s[4, 40:60] = EMPTY
    s[5, :] = EMPTY                                # an all-empty row
    out["ties"] = (s, 6, 4)
    # all rows empty: equal everywhere, linked nowhere
    out["all_empty"] = (np.full((5, 128), EMPTY, np.uint32), 1, 4)
    # overflow: row 0 has 9 partners, row 1 (equal to row 0) has 8, max_links 4
    s = np.stack([_row(B, rng) for _ in range(14)])
    for j in (1, 3, 4, 6, 7, 9, 10, 12, 13):
        s[j, 10:30] = s[0, 10:30]
    out["overflow"] = (s, 20, 4)
    out["overflow_1"] = (s, 20, 1)
    out["n1"] = (_row(256, rng)[None, :], 1, 8)
    # n = 65: the lanes of a second step; 0 - 64 linked across it, a triangle 10 - 30 - 64, 2 and 40 with 63
    s = np.stack([_row(256, rng) for _ in range(65)])
    s[64, :8] = s[0, :8]
    s[30, 100:110] = s[10, 100:110]
    s[64, 100:110] = s[10, 100:110]
    s[63, 200:207] = s[2, 200:207]
    s[63, 210:217] = s[40, 210:217]
    out["n65"] = (s, 7, 256)
    out["n65_cut"] = (s, 7, 3)
    s = np.stack([_row(512, rng) for _ in range(130)])
    s[::3, 500:512] = s[0, 500:512]
    s[5:9] = s[5]
    out["b512_n130"] = (s, 12, 64)
    return out


LINK_IDS = list(link_sets())


@functools.lru_cache(maxsize=None)
def expected_links(name):
    s, mm, ml = link_sets()[name]
    return orc.sketch_links(s, mm, ml)


def assert_links_equal(got, want, name):
    for what, g, w in zip(("degree", "links", "matches"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, what, g.shape, w.shape, g.dtype)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{name}: {what} differs at {bad[:5].tolist()}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"


def planted_sketches(n=1500, groups=30, buckets=256, seed=31):
    """n random sketches, the first 10 * groups of them in planted groups of 10: a group has 60 buckets of its own, a member holds the
    group's hashes in 30 .. 50 of them (two members share ~27); ~5 % empty buckets everywhere."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 0xFFFFFFF0, (n, buckets), dtype=np.uint32)
    centre = rng.integers(0, 0xFFFFFFF0, (groups, buckets), dtype=np.uint32)
    own = [rng.choice(buckets, 60, replace=False) for _ in range(groups)]
    for i in range(10 * groups):
        cols = rng.choice(own[i % groups], int(rng.integers(30, 51)), replace=False)
        s[i, cols] = centre[i % groups, cols]
    s[rng.random((n, buckets)) < 0.05] = EMPTY
    return s


# ---- the refusals: (what differs from a good call, the return code in the message)
U6 = unit_code("CCCTAA")[0]
SKETCH_REFUSALS = [
    (dict(code=unit_code("CCT")[0], m=3), "rc=-3"), (dict(code=0, m=33), "rc=-3"), (dict(code=unit_code("CCACCA")[0]), "rc=-3"),
    (dict(code=U6 | 1 << 12), "rc=-3"), (dict(buckets=32), "rc=-3"), (dict(buckets=192), "rc=-3"), (dict(buckets=1024), "rc=-3"),
    (dict(tails=[2]), "rc=-3"), (dict(begin=[-1]), "rc=-3"), (dict(begin=[50], end=[49]), "rc=-3"),
    (dict(lens=(2, 256, 1)), "rc=-3"), (dict(lens=(1, 255, 1)), "rc=-3"), (dict(lens=(1, 256, 2)), "rc=-3"),
    (dict(k=7), "rc=-5"), (dict(k=17), "rc=-5"), (dict(begin=[0], end=[16385]), "rc=-5"),
]
LINK_REFUSALS = [
    (dict(buckets=32), "rc=-3"), (dict(lens=(127, 2, 8, 8)), "rc=-3"), (dict(lens=(128, 1, 8, 8)), "rc=-3"), (dict(lens=(128, 2, 7, 8)), "rc=-3"),
    (dict(lens=(128, 2, 8, 9)), "rc=-3"),
    (dict(n=262145, lens=(262145 * 64, 262145, 262145 * 4, 262145 * 4)), "rc=-5"), (dict(min_match=0), "rc=-5"), (dict(min_match=65), "rc=-5"),
    (dict(max_links=0, lens=(128, 2, 0, 0)), "rc=-5"), (dict(max_links=257, lens=(128, 2, 514, 514)), "rc=-5"),
]


# ---- detection: planted chromosome ends
DETECT = {"CCCTAA": (41, 42), "AAACCCT": (43, 44), "ACGGATGTCTAACTTCTTGGTGT": (45, 46)}          # motif -> seeds (ONT, HiFi)
DETECT_IDS = [f"{m}_{e}" for m in DETECT for e in ("ONT", "HIFI")]
N_ENDS, PER_END, N_LONE, READ_LEN = 6, 12, 20, 6000
SPAN, K, BUCKETS, MIN_MATCH, MIN_KMERS, MIN_READS, MAX_LINKS = 2000, 12, 256, 6, 200, 3, 64          # the defaults of topsicle_amd.ends


@functools.lru_cache(maxsize=None)
def detection_reads(ident):
    """(reads, truth, tails, telomere lengths): 6 planted ends x 12 reads of 6000 bases -- 300 .. 3000 bases of the motif, then that
    end's random subtelomere, errors applied, either orientation -- and 20 reads whose subtelomere is their own.  truth[i] = the
    planted end 1 .. 6, 0 for the unrelated reads."""
    motif, err = ident.rsplit("_", 1)
    rng = np.random.default_rng(DETECT[motif][0 if err == "ONT" else 1])
    errors = synth.ONT if err == "ONT" else synth.HIFI
    subs = [rand(rng, READ_LEN + 600) for _ in range(N_ENDS)]
    reads, truth, tails, telo = [], [], [], []
    for e in list(range(1, N_ENDS + 1)) * PER_END + [0] * N_LONE:
        t = int(rng.integers(300, 3001))
        sub = subs[e - 1] if e else rand(rng, READ_LEN + 600)
        mol = mutate(rng, repeats(motif, t, int(rng.integers(0, len(motif)))) + sub, errors)[:READ_LEN]
        assert len(mol) == READ_LEN
        tail = int(rng.integers(0, 2))
        reads.append(stored_revcomp(mol) if tail else mol)
        truth.append(e)
        tails.append(tail)
        telo.append(t)
    return reads, truth, tails, telo


def detection_windows(ident, jitter_seed=0):
    """The windows a boundary caller would hand over: the planted boundary +- 300 (a caller is early as often as late)."""
    _reads, _truth, _tails, telo = detection_reads(ident)
    rng = np.random.default_rng(1000 + jitter_seed)
    begin = [max(0, t + int(rng.integers(-300, 301))) for t in telo]
    return begin, [min(b + SPAN, READ_LEN) for b in begin]


def groups_from(sketch, kept, links_fn):
    """(end per read, degree) by the rule of topsicle_amd.ends at its defaults, the links by `links_fn(sketch, min_match, max_links)`;
    the grouping is the oracle's (ends_oracle.groups)."""
    part = [i for i in range(len(kept)) if kept[i] >= MIN_KMERS]
    degree, links, _ = links_fn(sketch[part], MIN_MATCH, MAX_LINKS)
    edges = [(i, int(j)) for i in range(len(part)) for j in links[i] if j >= 0]
    end = [0] * len(kept)
    for p, g in zip(part, orc.groups(len(part), edges, MIN_READS)):
        end[p] = g
    return end, degree


def write_fasta(path, reads):
    with open(path, "w") as fh:
        fh.write("".join(f">read{i}\n{s}\n" for i, s in enumerate(reads)))


# ---- `--ends` end to end: what the CLI tests (host emulation and GPU) check
def check_cli_outputs(outdir, ident, phrases=(4,)):
    """end_reads_{k}.csv and ends_{k}.csv say what the planted set asks for: one row per read of telolengths_all.csv with a stored
    boundary, no group with reads of two planted ends, no unrelated read assigned, ends_{k}.csv the summary of end_reads_{k}.csv.
    Returns the planted reads that sit in their end's largest group."""
    import csv
    import os
    from topsicle_amd import ends
    _reads, truth, tails, _telo = detection_reads(ident)
    telo = {}
    for row in list(csv.reader(open(os.path.join(outdir, "telolengths_all.csv"))))[1:]:
        telo[(row[1], row[3])] = row[4]
    good = None
    for k in phrases:
        rows = list(csv.reader(open(os.path.join(outdir, f"end_reads_{k}.csv"))))
        assert rows[0] == ends.READ_HEADER
        rows = rows[1:]
        stored = [rid for (kk, rid), t in telo.items() if kk == str(k) and float(t) != 0]
        assert [r[1] for r in rows] == stored                               # run order, stored boundaries only
        by_group = {}
        for r in rows:
            i = int(r[1][4:])
            assert r[2] == ("reverse" if tails[i] else "forward") and float(r[3]) == float(telo[(str(k), r[1])])
            assert int(r[4]) == int(float(r[3])) and int(r[5]) == min(int(r[4]) + SPAN, 20000)
            g = int(r[7])
            if g:
                assert truth[i] != 0, f"unrelated read {i} was assigned"
                by_group.setdefault(g, []).append((truth[i], r))
                assert int(r[8]) >= 1 and int(r[9]) >= MIN_MATCH and int(r[6]) >= MIN_KMERS
        for g, mem in by_group.items():
            assert len({t for t, _ in mem}) == 1, f"group {g} mixes planted ends"
        sizes = [len(by_group[g]) for g in sorted(by_group)]
        assert sorted(by_group) == list(range(1, len(by_group) + 1)) and sizes == sorted(sizes, reverse=True) and min(sizes) >= MIN_READS
        groups = list(csv.reader(open(os.path.join(outdir, f"ends_{k}.csv"))))
        assert groups[0] == ends.GROUP_HEADER and len(groups) - 1 == len(by_group)
        for row in groups[1:]:
            mem = [r for _t, r in by_group[int(row[0])]]
            tl = np.array([float(r[3]) for r in mem])
            assert int(row[1]) == len(mem) and int(row[2]) == sum(r[2] == "forward" for r in mem) and int(row[2]) + int(row[3]) == len(mem)
            assert (int(row[4]), row[5], row[6], int(row[7])) == (int(tl.min()), "%.1f" % np.median(tl), "%.1f" % tl.mean(), int(tl.max()))
        best = {}
        for g, mem in by_group.items():
            best[mem[0][0]] = max(best.get(mem[0][0], 0), len(mem))
        good = sum(best.values()) if good is None else min(good, sum(best.values()))
    return good
