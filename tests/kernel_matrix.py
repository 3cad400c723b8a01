"""Shared rows and checkers of the scan-kernel matrix (tests/test_kernel_matrix.py on the host emulation,
tests/test_gpu_kernel_matrix.py on the MI355X).  Not collected by pytest: no test_ prefix.

A ROW is one scan configuration: a pattern table, the scan parameters, and the EXACT kernel the library must launch for
it on a batch without non-ACGT letters (`kernel`) and on one with them (`kernel_dirty`), as `kernel_info(slot)` names it
before " lds=".  Every one of the library's scan kernels (TPS_SCAN_KERNEL_DECL in csrc/tps_kernels.h) has rows on both
kinds of batch; the path rows on top put the tile paths of csrc/tps_plan.h on their edges: window shapes off the home
shape (q not a multiple of 8), jumps and min_size, the lw = 255 / 256 switch of the chain-corrected tiles, the raw rows'
pair table of fields, and the planner's limits.

`edge_reads` builds the reads a row needs: lengths on every window-count and tile boundary, telomere tracts on either
end, both ends or none, pure repeats (the largest counts), chains of a self-overlapping k-mer across lanes and tiles, both
strands; and dirty copies of two anchor reads, one per tail, with a non-ACGT letter on the first / last base, the step-1
heads' edges, a window's first and last base and a tile's first window's first and last base, placed in the coordinates of
the tail the read takes.  `check_scan` compares a scan with the C oracle (oracle/oracle.c) read by read and
window by window.
"""
from __future__ import annotations

import collections
import dataclasses

import numpy as np

import oracle_c as occ
import topsicle_oracle as orc
from topsicle_amd import allsteps, hiplib

NT = 64                       # lanes per wave (tps::NT): a fused tile holds NT * 8 window blocks
SUMS = hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS
RAW = SUMS | hiplib.F_STORE_RAW
COMP = str.maketrans("ACGTacgt", "TGCAtgca")

# the tables of the kernel families: (motif, k, flags).  Which kernel a table takes is the planner's choice (tps_plan.h
# plan_geometry, topsicle_hip.hip do_scan); the comments say why.
TABLES = {
    "plain": ("AACCGGTT", 6, SUMS),   # 16 k-mers, no self-overlap, k > 4: no pair table (the sixteenth pattern: p16_ok)
    "p": ("CCCTAA", 4, SUMS),         # k <= 4, no self-overlap: pair table of masks
    "r": ("CCCTAA", 4, RAW),          # ... with raw rows: per-pattern tiles (_s6r: pair table of fields at r = 0)
    "so": ("CCCTAA", 6, SUMS),        # self-overlap period 5 (CTAACC ...): chain-corrected sums tiles
    "sol": ("CCCTAA", 5, SUMS),       # period 4 (CTAAC ...): the low-period sums kernels
    "sor": ("CCCTAA", 5, RAW),        # period 4 with raw rows: per-pattern tiles with chain repairs
    "sorh": ("CCCTAA", 6, RAW),       # period 5 with raw rows, 4^6 table: 16-bit field indices (LUT_F16)
    "q": ("AAACCCT", 5, SUMS),        # k = 5, no self-overlap: 16-bit pair and single tables
}
SUFFIX = {"plain": "", "p": "p", "r": "r", "so": "so", "sol": "sol", "sor": "sor", "sorh": "sorh", "q": "q"}
GENERIC = "tps_scan_kernel"


@dataclasses.dataclass
class Row:
    id: str
    family: str                 # key of TABLES, or "sixteen" (TTTTAGGG at k = 6: 16 k-mers, one self-overlap period)
    W: int = 100
    s: int = 6
    t: int = 100
    M: int = 20000
    no_bp: int = 1000
    jump: int = 5
    min_size: int = 2
    kernel: str = ""            # exact kernel on a clean batch
    kernel_dirty: str = ""      # ... on a batch with non-ACGT letters ("" = the same)
    knobs: dict = dataclasses.field(default_factory=dict)     # tps_ctx_debug_option keys (force_generic)
    filt: bool = False          # a filtering row: min_len and the cutoff's min_count (compared with oracle_c.batch_ck)
    cutoff: float = 0.4
    min_len: int = 3000

    @property
    def motif(self):
        return "TTTTAGGG" if self.family == "sixteen" else TABLES[self.family][0]

    @property
    def k(self):
        return 6 if self.family == "sixteen" else TABLES[self.family][1]

    @property
    def flags(self):
        return SUMS if self.family == "sixteen" else TABLES[self.family][2]

    @property
    def raw(self):
        return bool(self.flags & hiplib.F_STORE_RAW)

    @property
    def patterns(self):
        return orc.kmer_table(self.motif, self.k)

    @property
    def q(self):
        return max(0, self.W - self.k) // self.s

    @property
    def tw(self):
        """Windows per fused tile (tps_plan.h: tw = (NT * 8 - q - 1) & ~1)."""
        return (NT * 8 - self.q - 1) & ~1

    def expected(self, dirty):
        return (self.kernel_dirty or self.kernel) if dirty else self.kernel

    def params(self):
        mc = allsteps.min_count_for_cutoff(self.cutoff, self.no_bp / len(self.motif), self.no_bp) if self.filt else -1
        return hiplib.make_params(no_bp=self.no_bp, min_len=self.min_len if self.filt else 0, min_count=mc, window=self.W,
                                  slide=self.s, trimfirst=self.t, maxlen=self.M, jump=self.jump, min_size=self.min_size,
                                  flags=self.flags)


def kname(fam, s):
    return "tps_scan_kernel_s%d%s" % (s, SUFFIX[fam])


def _rows():
    R = []
    # every family at every slide of its kernels, home window
    for fam in TABLES:
        for s in (5, 6, 7, 8):
            R.append(Row(f"{fam}_s{s}", fam, s=s, kernel=kname(fam, s)))
    # the default kernels' other slides (sums only, no self-overlap); slide 12 needs q = (W - k) / 12 >= 8
    for s in (3, 4, 9, 10, 11, 12):
        R.append(Row(f"plain_s{s}", "plain", s=s, W=110 if s == 12 else 100, kernel=kname("plain", s)))
        R.append(Row(f"p_s{s}", "p", s=s, kernel=kname("p", s)))
    # the generic kernel: the knob, a slide without a fused kernel, a sixteen-pattern self-overlap table on a dirty batch
    R.append(Row("p_s6_force_generic", "p", knobs={"force_generic": 1}, kernel=GENERIC))
    R.append(Row("so_s6_force_generic", "so", knobs={"force_generic": 1}, kernel=GENERIC))
    R.append(Row("p_s13", "p", s=13, W=120, kernel=GENERIC))
    R.append(Row("sixteen_s6", "sixteen", kernel=kname("so", 6), kernel_dirty=GENERIC))
    R.append(Row("sixteen_s8", "sixteen", s=8, kernel=kname("so", 8), kernel_dirty=GENERIC))
    # default sums tiles off the home shape (q % 8 != 0: the unpacked window phase)
    for fam in ("plain", "p", "q"):
        for s in (5, 6, 7, 8):
            for W in (93, 101, 157):
                R.append(Row(f"{fam}_s{s}_W{W}", fam, s=s, W=W, kernel=kname(fam, s)))
    # jump on the headline kernel; jump x min_size on one kernel of every other family
    for j in range(1, 14):
        if j != 5:
            R.append(Row(f"p_s6_j{j}", "p", jump=j, kernel=kname("p", 6)))
    for fam, s in (("plain", 7), ("r", 6), ("so", 6), ("sol", 5), ("sor", 8), ("sorh", 7), ("q", 6)):
        for j in (1, 3, 4, 8, 13):
            for ms in (1, 2, 4):
                R.append(Row(f"{fam}_s{s}_j{j}_m{ms}", fam, s=s, jump=j, min_size=ms, kernel=kname(fam, s)))
    # self-overlap sums: lw = 255 (chain-corrected tiles) and lw = 256 (flag-and-recount tile)
    for fam in ("so", "sol"):
        k = TABLES[fam][1]
        for W in (255 + k, 256 + k):
            R.append(Row(f"{fam}_s6_W{W}", fam, W=W, kernel=kname(fam, 6)))
    # raw rows off the home window (_s6r: no pair table of fields at r != 0)
    for fam in ("r", "sor", "sorh"):
        for W in (93, 157):
            R.append(Row(f"{fam}_s6_W{W}", fam, W=W, kernel=kname(fam, 6)))
    # planner parameters
    for nb in (300, 1400):
        R.append(Row(f"p_s6_nobp{nb}", "p", no_bp=nb, kernel=kname("p", 6)))
        R.append(Row(f"so_s6_nobp{nb}", "so", no_bp=nb, kernel=kname("so", 6)))
    for t in (0, 37):
        R.append(Row(f"p_s6_t{t}", "p", t=t, kernel=kname("p", 6)))
        R.append(Row(f"sor_s6_t{t}", "sor", t=t, kernel=kname("sor", 6)))
    R.append(Row("p_s6_M4000", "p", M=4000, kernel=kname("p", 6)))
    R.append(Row("sorh_s6_M4000", "sorh", M=4000, kernel=kname("sorh", 6)))
    # the largest no_bp / window that still plans a fused kernel, and the next one up (tps_plan.h: the two step-1 heads must fit
    # the tile buffer, 2 head_dw <= fused_seq_dw(slide); a window's far end must lie within the exchange halo, q / 8 + 2 < XLANES - NT)
    R.append(Row(f"p_s6_nobp{NOBP_MAX}", "p", no_bp=NOBP_MAX, kernel=kname("p", 6)))
    R.append(Row(f"p_s6_nobp{NOBP_MAX + 1}", "p", no_bp=NOBP_MAX + 1, kernel=GENERIC))
    R.append(Row(f"p_s6_W{W_MAX}", "p", W=W_MAX, kernel=kname("p", 6)))
    R.append(Row(f"p_s6_W{W_MAX + 1}", "p", W=W_MAX + 1, kernel=GENERIC))
    # filtering rows: min_len and the cutoff's min_count (pass, best_* and the step-1 decision against oracle_c.batch_ck)
    for fam in ("p", "so", "sor", "q"):
        R.append(Row(f"{fam}_s6_filter", fam, filt=True, kernel=kname(fam, 6)))
    return R


NOBP_MAX = 1537   # at slide 6, k = 4 (test_kernel_matrix.py::test_planner_boundaries re-derives both from the planner)
W_MAX = 675
ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}


def periods(p):
    return [d for d in range(1, len(p)) if all(p[i] == p[i + d] for i in range(len(p) - d))]


# --------------------------------------------------------------------------------------------- reads
def _tract(motif, n, rng, err=0.0):
    s = list((motif * (n // len(motif) + 2))[:n])
    for i in np.nonzero(rng.random(n) < err)[0]:
        s[i] = "ACGT"[int(rng.integers(4))]
    return "".join(s)


def _rand(n, rng):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, max(n, 0)))


def edge_lengths(row):
    """Read lengths on the window-count and tile edges of `row`: window counts 0, 1, 2, 6 .. 9, 16, 17, tw - 1 .. tw + 1,
    2 tw, 2 tw + 1, each exactly and once more with extra bases that do not make another window.  Every count gets ONE extra
    amount, cycling through 1 .. s - 1 over the counts (all pairs would be 13 (s - 1) reads: the 80-read batch holds them
    only at slide 5 and below), so every extra amount appears.  Then lengths around maxlen and below 2 no_bp (the two
    step-1 heads overlap)."""
    k, W, s, t, M = row.k, row.W, row.s, row.t, row.M
    tw = row.tw
    L_of = lambda n: t + W + (n - 1) * s
    out = [0, 1, k - 1, t + W - 1]
    extra = 1
    for n in (1, 2, 6, 7, 8, 9, 16, 17, tw - 1, tw, tw + 1, 2 * tw, 2 * tw + 1):
        out.append(L_of(n))
        if s > 1:
            out.append(L_of(n) + extra)
            extra = extra % (s - 1) + 1
    out += [M - 1, M, M + 1, 2 * M]
    out += [row.no_bp - 1, row.no_bp + 7, 2 * row.no_bp - 1]
    return out


Mark = collections.namedtuple("Mark", "kind tail pos x")    # a dirty copy's letter: read position pos, x in its tail's scanned string


def edge_reads(row, seed=0):
    """(clean reads, dirty copies, marks): the clean reads of `row`; copies of two anchor reads (one per tail) with one
    non-ACGT letter on an edge each -- `marks[i]` says which edge, in read and tail coordinates -- then lower-case stretches
    and one all-N read.  Deterministic in the row's table and shape (rows that differ only in jump / min_size / knobs share
    reads)."""
    rng = np.random.default_rng([seed, row.k, row.W, row.s, row.t, row.M, row.no_bp, sum(map(ord, row.motif))])
    motif = row.motif
    k, s, t, W, nb = row.k, row.s, row.t, row.W, row.no_bp
    clean = []
    for i, L in enumerate(edge_lengths(row)):
        mode = i % 4                     # 0: tract at the start, 1: at the end, 2: both ends (equal step-1 counts), 3: none
        if mode == 2 and L >= 2 * nb + 2 * k:
            tr = _tract(motif, nb + k, rng)
            seq = tr + _rand(L - 2 * len(tr), rng) + tr
        else:
            n = int(L * rng.uniform(0.2, 0.7)) if mode < 3 else 0
            tr = _tract(motif, n, rng, err=0.02)
            seq = tr + _rand(L - n, rng) if mode == 0 else _rand(L - n, rng) + tr
        seq = seq[:L]
        clean.append(seq if i % 2 == 0 else seq[::-1].translate(COMP))
    L2 = t + W + 2 * row.tw * s + s - 1
    clean.append(_tract(motif, L2, rng))                                   # one pure repeat: the largest counts
    clean.append(_tract(motif, t + W + (row.tw + 3) * s, rng)[::-1].translate(COMP))
    # chains of each self-overlap period across lane (8 s bases) and tile boundaries, with single-base deletions
    for p in sorted({p for p in row.patterns for _ in periods(p)})[:3]:
        d = periods(p)[0]
        body = list(_rand(L2, rng))
        marks = [t + row.tw * s - 3 * d, t + 8 * s * 3 - 2, t + 8 * s * 17 - 1, t + row.tw * s + 8 * s - 5]
        for m in marks:
            run = list(p[:d] * (2 * k + 8 * s // d))
            for _ in range(2):
                del run[int(rng.integers(len(run)))]
            body[m:m + len(run)] = run
        clean.append("".join(body)[:L2])
    # two anchor reads whose tail step 1 cannot miss: the motif's tract over the windows of the first three tiles, then a
    # random end longer than a step-1 head (the forward tail), and its reverse complement (the tract at the end: the reverse tail)
    fwd = _tract(motif, t + W + 2 * row.tw * s + 8 * s, rng, err=0.01) + _rand(nb + 8 * s, rng)
    anchors = [fwd, fwd[::-1].translate(COMP)]
    clean += anchors
    # dirty copies of the anchors: one non-ACGT letter on an edge, placed in the coordinates of the read's own tail (window w of
    # the scanned string holds its characters w s .. w s + W - 2: oracle.c reads W - 1 of them)
    dirty, marks = [], []
    letters = "NRn-YKWSNR"
    for tail, a in enumerate(anchors):
        L = len(a)
        for kind, pos in (("first base", 0), ("last base", L - 1), ("start head's last base", nb - 1),
                          ("end head's first base", L - nb), ("base before the end head", L - nb - 1)):
            marks.append(Mark(kind, tail, pos, None))
        nwin = hiplib.window_count(L, W, s, t, row.M)
        j = 3
        for kind, x in (("window 0's first base", 0), (f"window {j}'s first base", j * s), (f"window {j}'s last base", j * s + W - 2),
                        ("tile 1's first window's first base", row.tw * s), ("tile 1's first window's last base", row.tw * s + W - 2),
                        ("tile 2's first window's first base", 2 * row.tw * s)):
            if nwin and x <= (nwin - 1) * s + W - 2:
                marks.append(Mark(kind, tail, t + x if tail == 0 else L - 1 - t - x, x))
    for i, m in enumerate(marks):
        a = anchors[m.tail]
        dirty.append(a[:m.pos] + letters[i % len(letters)] + a[m.pos + 1:])
    # ... lower-case stretches, and one read of nothing but N
    longs = [x for x in clean if len(x) > t + W + (row.tw + 2) * s and len(x) > 2 * nb]
    for i, base in enumerate(longs[:3]):
        a = t + (i + 1) * 7 * s
        dirty.append(base[:a] + base[a:a + 60].lower() + base[a + 60:])
        marks.append(Mark("lower-case stretch", None, a, None))
    dirty.append("N" * (t + W + 40 * s))
    marks.append(Mark("all N", None, 0, None))
    return clean, dirty, marks


def tail_of(seq, row):
    """The tail step 1 picks for `seq` (oracle): 0 forward if the start head's best count is strictly larger, else 1 reverse."""
    cs, ce = occ.trc_counts(seq, row.patterns, row.no_bp)
    return 0 if max(cs) > max(ce) else 1


# --------------------------------------------------------------------------------------------- checks
_oracle_cache: dict = {}


def _oracle(row, seq):
    key = (tuple(row.patterns), row.W, row.s, row.t, row.M, row.no_bp, seq)
    hit = _oracle_cache.get(key)
    if hit is None:
        pats = row.patterns
        cs, ce = occ.trc_counts(seq, pats, row.no_bp)
        wins = {tail: occ.window_counts(seq, tail, pats, row.W, row.s, row.t, row.M) for tail in ("forward", "reverse")}
        hit = _oracle_cache[key] = (cs, ce, wins)
        if len(_oracle_cache) > 4096:
            _oracle_cache.clear()
    return hit


def _bkp_exact(sums, jump, min_size):
    b = orc.binseg_l2_exact(sums, jump, min_size)
    return -1 if b is None else b


def check_scan(out, row, reads, tag=""):
    """`out` = dict(results, sums, win_off, raw, c_start, c_end) of one scan of `reads` under `row` (a GPU scan or the
    emulation's); every field against the oracle.  Returns (reads, windows) compared."""
    pats = row.patterns
    P = len(pats)
    prm = row.params()
    res = out["results"]
    n = len(reads)
    assert len(res) == n
    nw = np.array([hiplib.window_count(len(x), row.W, row.s, row.t, row.M) for x in reads], np.int64)
    want_off = np.concatenate([[0], np.cumsum(nw)])
    assert np.array_equal(out["win_off"], want_off), (row.id, tag, "win_off")
    n_windows = 0
    tie = (res["flags"] & hiplib.RES_TIE) != 0
    for i, seq in enumerate(reads):
        cs, ce, wins = _oracle(row, seq)
        where = (row.id, tag, i, len(seq))
        assert out["c_start"][i].tolist() == cs and out["c_end"][i].tolist() == ce, where + ("step-1 counts",)
        r = res[i]
        bs, be = max(cs), max(ce)
        assert (r["best_start"], r["best_end"]) == (bs, be), where
        assert (r["best_start_idx"], r["best_end_idx"]) == (int(np.argmax(cs)), int(np.argmax(ce))), where
        tail = 0 if bs > be else 1
        assert r["tail"] == tail, where
        passes = len(seq) > prm.min_len and (be if tail else bs) > prm.min_count
        assert r["pass"] == int(passes), where
        lo, hi = want_off[i], want_off[i + 1]
        if not passes:
            assert r["n_win"] == 0 and r["bkp"] == -1, where
            # no kernel writes the windows of a read that does not pass: the downloads hand them out as zeros (include/topsicle_hip.h)
            assert not out["sums"][lo:hi].any(), where + ("S_w of a read that does not pass",)
            if row.raw:
                assert not out["raw"][lo:hi].any(), where + ("raw rows of a read that does not pass",)
            continue
        assert r["n_win"] == nw[i], where
        sums, raw = wins["reverse" if tail else "forward"]
        got = out["sums"][lo:hi]
        if not np.array_equal(got, sums):
            bad = int(np.nonzero(got != sums)[0][0])
            raise AssertionError(f"{where}: S_w differs first at window {bad} of {hi - lo}: got {got[bad]}, oracle {sums[bad]}")
        if row.raw:
            g = out["raw"][lo:hi]
            if not np.array_equal(g, raw):
                bad = np.argwhere(g != raw)[0]
                raise AssertionError(f"{where}: raw row differs first at window {bad[0]} pattern {bad[1]}: got {g[bad[0]]}, oracle {raw[bad[0]]}")
        n_windows += int(hi - lo)
        assert r["bkp"] == _bkp_exact(sums, row.jump, row.min_size), where + ("bkp", int(r["bkp"]))
        if tie[i]:
            want, _ = occ.binseg_l2_y(sums.astype(np.float64) / P, row.jump, row.min_size)    # (oracle.c's float64 Binseg)
            assert out["bkp_resolved"][i] == (-1 if want is None else want), where + ("tie",)
    if row.filt:
        bases, offsets = hiplib.pack_reads(reads)
        o, ck = occ.batch_ck(bases, offsets, pats, len(row.motif), row.no_bp, row.min_len, row.cutoff, row.W, row.s, row.t,
                             row.M, both_tails=False)
        assert np.array_equal(res["pass"], o[:, 0]), (row.id, tag, "pass")
        longer = np.array([len(x) > row.min_len for x in reads])
        assert np.array_equal(res["tail"][longer], o[longer, 1]), (row.id, tag)
        idx = np.where(res["tail"] == 0, res["best_start_idx"], res["best_end_idx"])
        best = np.where(res["tail"] == 0, res["best_start"], res["best_end"])
        assert np.array_equal(idx[longer], o[longer, 2]) and np.array_equal(best[longer], o[longer, 3]), (row.id, tag)
        p = res["pass"].astype(bool)
        assert p.any() and (~p).any(), (row.id, "a filtering row must keep some reads and drop others")
        assert np.array_equal(res["n_win"][p], o[p, 4]), (row.id, tag)
        assert np.array_equal(out["bkp_resolved"][p], o[p, 5]), (row.id, tag, "bkp vs float64")
        got = occ.checksums(out["sums"], out["win_off"])
        assert np.array_equal(got[p], ck[p, 0]), (row.id, tag, "S_w checksums")
    return n, n_windows


def resolve_with(sums, win_off, res, P, jump, min_size):
    """bkp with the RES_TIE reads handed to ruptures' float64 arithmetic (hiplib.resolve_ties, from downloaded S_w)."""
    b = res["bkp"].copy()
    for i in np.nonzero((res["flags"] & hiplib.RES_TIE) != 0)[0]:
        b[i] = hiplib.binseg_l2_float64(np.asarray(sums[win_off[i]:win_off[i + 1]], np.float64) / P, jump, min_size)
    return b


def same_outputs(a, b, reads_a, reads_b, tag):
    """Byte identity of two scans' outputs for the reads `reads_a` of scan a and `reads_b` of scan b (index arrays)."""
    ra, rb = a["results"][reads_a], b["results"][reads_b]
    assert ra.tobytes() == rb.tobytes(), (tag, "results")
    assert np.array_equal(a["c_start"][reads_a], b["c_start"][reads_b]) and np.array_equal(a["c_end"][reads_a], b["c_end"][reads_b]), (tag, "step-1")
    for ia, ib in zip(reads_a, reads_b):         # (every read: those that do not pass come down as zeros)
        sa = a["sums"][a["win_off"][ia]:a["win_off"][ia + 1]]
        sb = b["sums"][b["win_off"][ib]:b["win_off"][ib + 1]]
        assert sa.tobytes() == sb.tobytes(), (tag, "sums", int(ia))
        if a.get("raw") is not None:
            xa = a["raw"][a["win_off"][ia]:a["win_off"][ia + 1]]
            xb = b["raw"][b["win_off"][ib]:b["win_off"][ib + 1]]
            assert xa.tobytes() == xb.tobytes(), (tag, "raw", int(ia))
