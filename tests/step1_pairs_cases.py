"""Cases of step 1 in the pair-table kernels (csrc/tps_device.h: trc_decide_pairs) for test_step1_pairs.py (the host emulation)
and test_gpu_step1_pairs.py (the MI355X): small batches scanned with F_STEP1 alone, every read against the oracle's step-1
counts and decision, and the route the kernel must take for it.

The new count splits a head's npos = n - k + 1 start positions into full lanes of 32 and a remainder of npos % 32, looks two
positions up at a time and adds masks in bit planes, so the reads sit on those edges: npos at and beside the multiples of 32,
heads shorter than a k-mer, heads that overlap or abut, occurrences on the last counted position, on the first one behind it
and on both sides of a lane boundary (in both heads), and the densest heads a table without self-overlap allows (a pattern
every k bases: 255 occurrences at the bound npos = 255 k, just over it the old route)."""
import dataclasses

import numpy as np

import oracle_c as occ
import topsicle_oracle as orc
from topsicle_amd import hiplib

PAIRS, PACKED, HIST = 12, 13, 14          # emulation counters of the step-1 routes (csrc/tps_wave.h)

K3 = ["CCT", "CTA", "TAA", "AAC", "ACC", "GGA", "GAT", "ATT", "TTG", "TGG"]          # k = 3 without self-overlap (no p[0] == p[2])
TABLES = {
    "k4_P12": orc.kmer_table("CCCTAA", 4),       # three words of count bytes
    "k4_P14": orc.kmer_table("CCCTAAA", 4),      # four words
    "k4_P3": ["CCCT", "CTAA", "AACC"],           # one word
    "k5_P14": orc.kmer_table("AAACCCT", 5),      # 16-bit entries (_s*q)
    "k3_P10": K3,
    "k2_P3": ["AC", "CA", "GT"],                 # k = 2: a lane could count 17 of a pattern, more than four planes hold -- the old route
}


@dataclasses.dataclass
class Case:
    id: str
    table: str
    slide: int = 6
    no_bp: int = 1000
    reads: list = None
    kernel_suffix: str = "p"

    @property
    def patterns(self):
        return TABLES[self.table]

    @property
    def k(self):
        return len(self.patterns[0])

    def params(self):
        # a cutoff in the middle of the counts, so that `pass` is 0 for some reads and 1 for others
        return hiplib.make_params(no_bp=self.no_bp, min_len=0, min_count=self.no_bp // 40, window=110 if self.slide == 12 else 100,
                                  slide=self.slide, trimfirst=100, maxlen=20000, flags=hiplib.F_STEP1)


def _rand(n, rng):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, max(n, 0)))


def _with(bg, at, pat):
    """`bg` with `pat` written over it at position `at`."""
    return bg[:at] + pat + bg[at + len(pat):]


def head_edge_lengths(k, no_bp):
    """Read lengths (L <= no_bp: the head is the read) that put npos = L - k + 1 at and beside the lane boundaries, with an odd
    and an even remainder, and the shortest reads."""
    out = list(range(1, k + 2))
    for m in (1, 2, 7, no_bp // 32 - 1, (no_bp - k + 1) // 32):
        for npos in (32 * m - 1, 32 * m, 32 * m + 1, 32 * m + 14, 32 * m + 15):
            L = npos + k - 1
            if k < L <= no_bp:
                out.append(L)
    return sorted(set(out))


def reads_for(table, no_bp, rng, dirty=False):
    pats = TABLES[table]
    k = len(pats[0])
    motif = {"k4_P12": "CCCTAA", "k4_P14": "CCCTAAA", "k4_P3": "CCCTAA", "k5_P14": "AAACCCT", "k3_P10": "CCTAA", "k2_P3": "ACGT"}[table]
    npos = no_bp - k + 1
    full = npos // 32
    reads = []
    # head ends
    for L in head_edge_lengths(k, no_bp) + [no_bp - 1, no_bp, no_bp + 1, no_bp + 3, no_bp + 4, no_bp + no_bp // 2, 2 * no_bp, 2 * no_bp + 77]:
        tel = (motif * (L // len(motif) + 2))[:L]
        reads.append(_rand(L, rng))
        reads.append(tel)                                        # perfect telomere: both heads, every pattern at its densest
        reads.append(_with(_rand(L, rng), 0, tel[: L // 2]))      # forward tail
        reads.append(_with(_rand(L, rng), L - L // 2, tel[: L // 2]))
    # boundary occurrences, start head: the last counted position, the first uncounted one, both sides of the last full lane's
    # end and of lane 0's; the same on the reversed end head (the read's last bases, reversed, are the head)
    bg = "AG" * (no_bp + 40)
    for pat in (pats[0], pats[-1]):
        for at in (npos - 1, npos, 32 * full - 1, 32 * full, 31, 32, 0, 1):
            if at < 0:
                continue
            head = _with(bg, at, pat)[: no_bp + 16]
            reads.append(head + _rand(no_bp + 50, rng))                       # start head
            reads.append(_rand(no_bp + 50, rng) + head[::-1])                 # end head (reversed)
    # the densest heads: a pattern every k bases
    for pat in (pats[0], pats[1]):
        reads.append(pat * (2 * no_bp // k + 3))
        reads.append(_rand(37, rng) + pat * (2 * no_bp // k))
    if dirty:
        # a non-ACGT letter inside a head: that read takes the old route, its neighbours do not
        n = len(reads)
        for i in range(0, n, 7):
            seq = reads[i]
            if len(seq) > 40:
                at = 20 if (i // 7) % 2 == 0 else len(seq) - 21
                reads[i] = seq[:at] + "N" + seq[at + 1:]
    return reads


def _cases():
    rng = np.random.default_rng(1212)
    C = []
    # tables (slide 6) and slides (CCCTAA, k = 4; the k = 5 table's kernels exist for slides 5 .. 8)
    for s in (3, 6, 7, 12):
        C.append(Case(f"k4_P12_s{s}", "k4_P12", slide=s, reads=reads_for("k4_P12", 1000, rng)))
    for s in (6, 7):
        C.append(Case(f"k5_P14_s{s}", "k5_P14", slide=s, reads=reads_for("k5_P14", 1000, rng), kernel_suffix="q"))
    C.append(Case("k4_P14_s6", "k4_P14", reads=reads_for("k4_P14", 1000, rng)))
    C.append(Case("k4_P3_s6", "k4_P3", reads=reads_for("k4_P3", 1000, rng)))
    # no_bp: heads of 64, 65 and 997 bases; the bound npos = 255 k (no_bp 1023: CCCT every 4 bases is counted 255 times) and
    # the first head over it (1024: the old route)
    for nb in (64, 65, 997, 1023, 1024):
        C.append(Case(f"k4_P12_nobp{nb}", "k4_P12", no_bp=nb, reads=reads_for("k4_P12", nb, rng)))
    # k = 3: 700-base heads are inside the bound (a pattern every 3 bases: a lane counts up to 11), 1000-base heads are not
    C.append(Case("k3_P10_nobp700", "k3_P10", no_bp=700, reads=reads_for("k3_P10", 700, rng)))
    C.append(Case("k3_P10_nobp1000", "k3_P10", no_bp=1000, reads=reads_for("k3_P10", 1000, rng)))
    C.append(Case("k2_P3_nobp400", "k2_P3", no_bp=400, reads=reads_for("k2_P3", 400, rng)))
    # a read with N in a head beside clean ones
    C.append(Case("k4_P12_s6_dirty", "k4_P12", reads=reads_for("k4_P12", 1000, rng, dirty=True)))
    C.append(Case("k5_P14_s6_dirty", "k5_P14", reads=reads_for("k5_P14", 1000, rng, dirty=True), kernel_suffix="q"))
    return C


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


def is_dirty(case):
    return any(set(x) - set("ACGT") for x in case.reads)


def expected_route(case, seq):
    """PAIRS where trc_decide_pairs must run: a clean read, at most 15 patterns of at least 3 letters, npos <= min(1024, 255 k)."""
    npos = min(len(seq), case.no_bp) - case.k + 1
    clean = not (set(seq) - set("ACGT"))
    return PAIRS if clean and len(case.patterns) <= 15 and case.k >= 3 and npos <= min(1024, 255 * case.k) else None


_ref: dict = {}


def reference(case):
    """[(c_start, c_end)] of the case's reads from the C oracle, computed once."""
    if case.id not in _ref:
        _ref[case.id] = [occ.trc_counts(seq, case.patterns, case.no_bp) for seq in case.reads]
    return _ref[case.id]


def check(case, res, c_start, c_end, tag):
    prm = case.params()
    n_pass = 0
    for i, (seq, (cs, ce)) in enumerate(zip(case.reads, reference(case))):
        where = (case.id, tag, i, len(seq))
        assert c_start[i].tolist() == cs and c_end[i].tolist() == ce, where + ("counts", c_start[i].tolist(), cs, c_end[i].tolist(), ce)
        r = res[i]
        bs, be = max(cs), max(ce)
        assert (r["best_start"], r["best_end"]) == (bs, be), where
        assert (r["best_start_idx"], r["best_end_idx"]) == (int(np.argmax(cs)), int(np.argmax(ce))), where
        tail = 0 if bs > be else 1
        assert r["tail"] == tail, where
        passes = len(seq) > prm.min_len and (be if tail else bs) > prm.min_count
        assert r["pass"] == int(passes), where
        n_pass += int(passes)
    return n_pass


def check_shapes(case):
    """The case's reads are on the edges they claim (oracle only)."""
    k, nb, pats = case.k, case.no_bp, case.patterns
    ref = reference(case)
    npos_seen = {min(len(x), nb) - k + 1 for x in case.reads}
    for m in (1, 2):
        if 32 * m + 1 + k - 1 <= nb:
            assert {32 * m - 1, 32 * m, 32 * m + 1} <= npos_seen
    assert any(v <= 0 for v in npos_seen) and 1 in npos_seen and 2 in npos_seen
    # the densest read: its pattern every k bases, counted on every k-th position of the head
    assert max(max(cs) for cs, _ in ref) == nb // k
    # an occurrence on the last counted position counts, one position later it does not (start head and end head)
    bg = "AG" * (nb + 40)
    npos = nb - k + 1
    for pat in (pats[0], pats[-1]):
        p = pats.index(pat)
        a = occ.trc_counts(_with(bg, npos - 1, pat)[: nb + 16] + "AG" * 40, pats, nb)[0][p]
        b = occ.trc_counts(_with(bg, npos, pat)[: nb + 16] + "AG" * 40, pats, nb)[0][p]
        assert a == b + 1
