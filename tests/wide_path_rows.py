"""Shared rows and checkers of the wide-table kernel's path matrix (tests/test_wide_paths.py on the host emulation,
tests/test_gpu_wide_paths.py on the MI355X).  Not collected by pytest: no test_ prefix.  Built like tests/kernel_matrix.py.

A ROW is one scan configuration of tps_scan_kernel_wide (csrc/tps_wide.h): a pattern table, W, s, t, M, no_bp, jump,
min_size, min_len, min_count, the flags, and the LDS plan plan_wide (csrc/tps_wide_plan.h) must give it -- `tp_cap` positions
per tile and `tw` windows per tile, as literals: a change of plan is seen.  The rows leave the one shape every older wide test
has (no_bp = 1000, windows of 60 to 300: tp_cap = 4096) in every direction the plan can go: tiles grown by the window and by
the step-1 head, tw = 1, tw below a wave, tw rounded to whole waves, the capacity boundary of the device's own LDS budget
(`boundary_rows`: derived from the planner, not literals), byte counters at 255, windows around lw1 = W - k, tables of
k = 1, 2, 3, heads around k and around a tile, strict filters, jump x min_size, dirty letters on the edges of a tile's staged
range.  `reads_of` builds a row's reads, `check_scan` compares a scan with oracle/oracle.c field by field.
"""
from __future__ import annotations

import dataclasses
import re
import struct

import numpy as np

import oracle_c as occ
import topsicle_oracle as orc
import wide_cases
from topsicle_amd import hiplib

NT = 64
FULL = hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS
RAW = FULL | hiplib.F_STORE_RAW
TAILS = hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_TAILS_IN | hiplib.F_STORE_SUMS | hiplib.F_STORE_RAW
STEP1 = hiplib.F_STEP1
E_CAPACITY = -5               # TPS_E_CAPACITY
WIDE = "tps_scan_kernel_wide"
COMP = str.maketrans("ACGTacgt", "TGCAtgca")

_P64 = wide_cases.made_up_tables()["p64"]
# name -> (pattern list, the string whose repeats make a tract of the table's k-mers)
TABLES = {
    "m23k21": (orc.kmer_table(wide_cases.MOTIFS[23], 21), wide_cases.MOTIFS[23]),      # P = 46; 14 k-mers begin and end with the same letter (period k - 1)
    "m32k32": (orc.kmer_table(wide_cases.MOTIFS[32], 32), wide_cases.MOTIFS[32]),      # P = 64, k = 32
    "acac16": (orc.kmer_table("AC" * 10, 16), "AC"),                                   # P = 4, every k-mer periodic (n_so = 4)
    "a20k18": (orc.kmer_table("A" * 20, 18), "A"),                                     # P = 2, homopolymers (n_so = 2)
    "p64": (_P64, "".join(_P64[:6])),                                                  # 64 random 20-mers, no complements
    "k1": (["A", "T"], "A"),
    "k2": (["AA", "TT", "AC", "GT"], "AC"),                                            # AA, TT walk; AC, GT slide
    "k3": (orc.kmer_table("CCCTAA", 3), "CCCTAA"),                                     # P = 12; CCC, GGG walk
}


@dataclasses.dataclass
class Row:
    id: str
    table: str
    W: int = 100
    s: int = 6
    t: int = 100
    M: int = 0                  # 0: room for 2 tw + 2 windows, 67 at least (the edge reads put lengths around it)
    no_bp: int = 1000
    jump: int = 5
    min_size: int = 2
    min_len: int = 0
    min_count: int = 0
    flags: int = RAW
    tp_cap: int = 4096          # the plan the row must get
    tw: int = 640
    reads: str = "edge"         # which builder of reads_of
    unit: str = ""              # the tract's unit, if not the table's
    filt: tuple = ()            # ("count" | "len", d): min_count / min_len = the anchor read's best count / length, minus d
    want_255: bool = False      # the raw rows must hold a 255
    refuse: int = 0             # a refusal row: the error code the scan must fail with

    def __post_init__(self):
        if self.M == 0:
            self.M = self.t + self.W + max(2 * self.tw + 1, 66) * self.s + 1

    @property
    def patterns(self):
        return TABLES[self.table][0]

    @property
    def k(self):
        return len(self.patterns[0])

    @property
    def raw(self):
        return bool(self.flags & hiplib.F_STORE_RAW)

    def params(self, min_len=None, min_count=None):
        return hiplib.make_params(no_bp=self.no_bp, min_len=self.min_len if min_len is None else min_len,
                                  min_count=self.min_count if min_count is None else min_count, window=self.W, slide=self.s,
                                  trimfirst=self.t, maxlen=self.M, jump=self.jump, min_size=self.min_size, flags=self.flags)


def _rows():
    R = []
    # ---- tile size: by the window (W - 1 = 4095, 4096, 4097, ~5000) ...
    R.append(Row("base_m23", "m23k21"))
    R.append(Row("base_acac", "acac16"))
    R.append(Row("W4096_s1", "a20k18", W=4096, s=1, tw=2))
    R.append(Row("W4096_s23", "a20k18", W=4096, s=23, tw=1))
    R.append(Row("W4097_s23_a20", "a20k18", W=4097, s=23, tw=1))
    R.append(Row("W4097_s23_m23", "m23k21", W=4097, s=23, tw=1, reads="few"))
    R.append(Row("W4098_s23", "a20k18", W=4098, s=23, tp_cap=4160, tw=3))
    R.append(Row("W4101_s2", "p64", W=4101, s=2, tp_cap=4160, tw=31, reads="few"))
    R.append(Row("W5001_s23_nobp4500", "m32k32", W=5001, s=23, no_bp=4500, tp_cap=5056, tw=3, reads="few"))        # W - 1 > no_bp > 4096
    R.append(Row("W4501_s23_nobp6000", "m23k21", W=4501, s=23, no_bp=6000, tp_cap=6016, tw=64, reads="few"))      # no_bp > W - 1 > 4096
    # ... and by the step-1 head (tw rounded down to whole waves)
    R.append(Row("nobp4096", "m23k21", no_bp=4096))
    R.append(Row("nobp4097", "m23k21", no_bp=4097, tp_cap=4160, tw=640))
    R.append(Row("nobp8000", "m23k21", no_bp=8000, tp_cap=8000, tw=1280))
    R.append(Row("nobp8000_acac_sums", "acac16", no_bp=8000, tp_cap=8000, tw=1280, flags=FULL, reads="few"))
    R.append(Row("nobp8000_tails_in", "m23k21", no_bp=8000, flags=TAILS))                 # without STEP1 no_bp does not count
    R.append(Row("nobp8000_step1", "acac16", no_bp=8000, tp_cap=8000, tw=1280, flags=STEP1, reads="few"))
    # ---- window shapes around lw1 = W - k
    for tab in ("m23k21", "acac16"):
        k = len(TABLES[tab][0][0])
        R.append(Row(f"{tab}_W10", tab, W=10, tw=640))                                     # W < k: lw1 = 0
        R.append(Row(f"{tab}_Wk", tab, W=k, tw=640))                                       # lw1 = 0
        R.append(Row(f"{tab}_Wk1", tab, W=k + 1, tw=640))                                  # lw1 = 1
        R.append(Row(f"{tab}_W{k + 19}_s25", tab, W=k + 19, s=25, tw=128))                 # slide > lw1
        R.append(Row(f"{tab}_W{k + 19}_s19", tab, W=k + 19, s=19, tw=192))                 # slide = lw1
        R.append(Row(f"{tab}_W{k + 19}_s6", tab, W=k + 19, s=6, tw=640))                   # slide < lw1
    # ---- tables of k = 1, 2, 3, and the byte counters at 255
    R.append(Row("k1_W256_A", "k1", W=256, reads="c255", want_255=True))                   # (W - 1) / k = 255: slid counters
    R.append(Row("k1_W256_AT", "k1", W=256, reads="c255", unit="AT"))
    R.append(Row("k1_W257", "k1", W=257, reads="c255", refuse=E_CAPACITY))
    R.append(Row("k2_W511_AC", "k2", W=511, reads="c255", want_255=True, tw=576))          # AC slides
    R.append(Row("k2_W511_A", "k2", W=511, reads="c255", unit="A", want_255=True, tw=576))  # AA walks
    R.append(Row("k2_W512_AC", "k2", W=512, s=7, reads="c255", want_255=True, tw=512))
    R.append(Row("k2_W513", "k2", W=513, reads="c255", refuse=E_CAPACITY))
    R.append(Row("k1_edge", "k1", W=60, s=5, tw=768))
    R.append(Row("k2_edge", "k2", W=100, s=7, tw=512))
    R.append(Row("k3_edge", "k3"))
    R.append(Row("k3_W300_s7", "k3", W=300, s=7, tw=512, reads="few"))
    # ---- step-1 heads: around k, around a wave, around a tile; step 1 alone and the full scan.  min_count = -1: every read with
    # a base passes, so the full rows count windows whatever the heads hold
    for tab in ("m23k21", "acac16"):
        k = len(TABLES[tab][0][0])
        for nb in (1, k - 1, k, k + 1, 63, 64, 65, 999, 4097):
            plan = dict(tp_cap=4160) if nb == 4097 else {}
            R.append(Row(f"{tab}_head{nb}_step1", tab, no_bp=nb, flags=STEP1, reads="heads", min_count=-1, **plan))
            R.append(Row(f"{tab}_head{nb}_full", tab, no_bp=nb, flags=RAW, reads="heads", min_count=-1, **plan))
    # ---- strict filters: min_count / min_len on the anchor read's own best count / length, and one less
    for tab in ("m23k21", "acac16"):
        for what in ("count", "len"):
            for d in (0, 1):
                R.append(Row(f"{tab}_filter_{what}_{d}", tab, reads="filter", filt=(what, d), flags=FULL))
    # ---- change point: jump x min_size
    for j in (1, 3, 8, 13):
        for ms in (1, 2, 4):
            R.append(Row(f"binseg_j{j}_m{ms}", "m23k21" if (j + ms) % 2 else "acac16", jump=j, min_size=ms, reads="binseg", flags=FULL))
    # ---- dirty letters on the edges of a tile's staged range and of the 4097-base heads
    R.append(Row("dirty_m23", "m23k21", no_bp=4097, tp_cap=4160, tw=640, reads="dirty"))
    R.append(Row("dirty_acac_s23", "acac16", W=200, s=23, no_bp=4097, tp_cap=4160, tw=128, reads="dirty"))
    return R


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
SCAN_ROWS = [r for r in ROWS if not r.refuse]
BOUNDARY_TABLES = ("k1", "acac16", "m23k21")    # n_so = 0, 4 and 14


def boundary_rows(budget_bytes, plan):
    """The capacity boundary at an LDS budget: for tables with 0, 4 and 14 self-overlapping groups, the largest no_bp
    (a multiple of 64, found by bisection over `plan(patterns, prm, budget_bytes)` = emu_wide_driver.plan) the plan accepts -- a
    scanning row -- and that value plus 64 -- a refusal row.  Returns [(accepted row, refused row, accepted plan)]."""
    out = []
    for tab in BOUNDARY_TABLES:
        def ok(nb):
            return "error" not in plan(TABLES[tab][0], Row("x", tab, no_bp=nb, M=30000).params(), budget_bytes)
        lo, hi = 4096 // 64, 32768 // 64 + 1            # accepted, refused (WIDE_TP_MAX + 64 is refused by its own rule)
        assert ok(lo * 64) and not ok(hi * 64)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if ok(mid * 64):
                lo = mid
            else:
                hi = mid
        nb = lo * 64
        pl = plan(TABLES[tab][0], Row("x", tab, no_bp=nb, M=30000).params(), budget_bytes)
        acc = Row(f"{tab}_nobp{nb}_largest", tab, no_bp=nb, M=30000, tp_cap=pl["tp_cap"], tw=pl["tw"], reads="capacity")
        ref = Row(f"{tab}_nobp{nb + 64}_refused", tab, no_bp=nb + 64, M=30000, reads="capacity", refuse=E_CAPACITY)
        out.append((acc, ref, pl))
    return out


def error_code(exc):
    """The TPS_E_* code inside a TopsicleHipError of the library ("error -5:") or of the emulation's driver ("rc=-5:")."""
    m = re.search(r"(?:error |rc=)(-?\d+):", str(exc))
    return int(m.group(1)) if m else None


# --------------------------------------------------------------------------------------------- reads
def _tract(unit, n, rng, err=0.0):
    s = list((unit * (n // len(unit) + 2))[:n])
    for i in np.nonzero(rng.random(n) < err)[0]:
        s[i] = "ACGT"[int(rng.integers(4))]
    return "".join(s)


def _rand(n, rng):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, max(n, 0)))


def L_of(row, n):
    """The shortest read with n >= 1 windows."""
    return row.t + row.W + (n - 1) * row.s


def edge_lengths(row):
    """Like kernel_matrix.edge_lengths: window counts 0, 1, 2, 63, 64, 65, tw - 1, tw, tw + 1, 2 tw, 2 tw + 1, each exactly and
    once more with extra bases (cycling through 1 .. s - 1) that make no further window; lengths around maxlen; the heads'
    no_bp - 1, no_bp, no_bp + 1 and 2 no_bp - 1 (the two heads overlap by all but one base)."""
    k, s, M, nb, tw = row.k, row.s, row.M, row.no_bp, row.tw
    out = [0, 1, k - 1, k, row.t + row.W - 1]
    extra = 1
    for n in (1, 2, 63, 64, 65, tw - 1, tw, tw + 1, 2 * tw, 2 * tw + 1):
        if n < 1:
            continue
        out.append(L_of(row, n))
        if s > 1:
            out.append(L_of(row, n) + extra)
            extra = extra % (s - 1) + 1
    out += [M - 1, M, M + 1, M + M // 2]
    out += [nb - 1, nb, nb + 1, 2 * nb - 1]
    return list(dict.fromkeys(x for x in out if x >= 0))


def _placed(row, lengths, rng, err=0.02):
    """Reads of the given lengths: tract at the start, at the end, at both ends (equal heads) or none, on both strands --
    every other read reversed, with the complement (the motif tables hold it) or without (the made-up ones do not)."""
    unit = row.unit or TABLES[row.table][1]
    k, nb = row.k, row.no_bp
    out = []
    for i, L in enumerate(lengths):
        mode = i % 4
        if mode == 2 and L >= 2 * nb + 2 * k:
            tr = _tract(unit, nb + k, rng)
            seq = tr + _rand(L - 2 * len(tr), rng) + tr
        else:
            n = int(L * rng.uniform(0.2, 0.7)) if mode < 3 else 0
            tr = _tract(unit, n, rng, err=err)
            seq = tr + _rand(L - n, rng) if mode == 0 else _rand(L - n, rng) + tr
        seq = seq[:L]
        if i % 2:
            seq = seq[::-1].translate(COMP) if i % 4 == 1 else seq[::-1]
        out.append(seq)
    return out


@dataclasses.dataclass
class Mark:
    kind: str
    tail: int
    pos: int        # read position of the letter
    x: int | None   # ... and its place in the tail's scanned string (None: a head's base)


def _anchors(row, rng):
    """Two reads whose tail step 1 cannot miss: a tract over the windows of tiles 0, 1 and the start of tile 2, then a random end
    longer than a head (the forward tail); reversed, with the complement, the reverse tail."""
    unit = row.unit or TABLES[row.table][1]
    fwd = _tract(unit, row.t + row.W + 2 * row.tw * row.s + 8 * row.s, rng, err=0.01) + _rand(row.no_bp + 8 * row.s, rng)
    return [fwd, fwd[::-1].translate(COMP)]


def dirty_reads(row):
    """(reads, marks): the two anchors, then copies of them with ONE non-ACGT letter each (marks[i] is reads[2 + i]'s), then one
    read of nothing but N.  Places, in the coordinates of the tail the anchor takes: the first and last base of tile 1's staged
    range, the last base of the window that ends tile 0, window 0's first base; the first and last base of either head."""
    rng = _rng(row)
    anchors = _anchors(row, rng)
    tw, s, W, t, nb = row.tw, row.s, row.W, row.t, row.no_bp
    marks = []
    for tail, a in enumerate(anchors):
        L = len(a)
        for kind, pos in (("start head's first base", 0), ("start head's last base", nb - 1), ("end head's first base", L - nb),
                          ("end head's last base", L - 1), ("base before the end head", L - nb - 1)):
            marks.append(Mark(kind, tail, pos, None))
        for kind, x in (("window 0's first base", 0), ("tile 0's last window's last base", (tw - 1) * s + W - 2),
                        ("tile 1's first staged base", tw * s), ("tile 1's last staged base", tw * s + (tw - 1) * s + W - 2),
                        ("tile 2's first staged base", 2 * tw * s)):
            marks.append(Mark(kind, tail, t + x if tail == 0 else L - 1 - t - x, x))
    letters = "NRn-YKWSNR"
    reads = list(anchors)
    for i, m in enumerate(marks):
        a = anchors[m.tail]
        reads.append(a[:m.pos] + letters[i % len(letters)] + a[m.pos + 1:])
    reads.append("N" * (t + W + 40 * s))
    return reads, marks


def _rng(row):
    return np.random.default_rng([row.k, row.W, row.s, row.t, row.M, row.no_bp, len(row.patterns), sum(map(ord, row.unit or row.table))])


_reads_cache: dict = {}


def reads_of(row):
    """The reads of `row`, deterministic in its table and shape (rows that differ in jump / min_size / filters share reads)."""
    key = (row.table, row.unit, row.W, row.s, row.t, row.M, row.no_bp, row.tw, row.reads, row.jump if row.reads == "binseg" else 0,
           row.min_size if row.reads == "binseg" else 0)
    hit = _reads_cache.get(key)
    if hit is None:
        hit = _reads_cache[key] = _build_reads(row)
    return hit


def _build_reads(row):
    rng = _rng(row)
    unit = row.unit or TABLES[row.table][1]
    k, s, t, W, nb, tw = row.k, row.s, row.t, row.W, row.no_bp, row.tw
    if row.reads == "edge":
        reads = _placed(row, edge_lengths(row), rng)
        reads.append(_tract(unit, L_of(row, 2 * tw) + s - 1, rng))                       # a pure repeat: the largest counts
        reads.append(_tract(unit, L_of(row, tw + 3), rng)[::-1].translate(COMP))
        return reads
    if row.reads == "few":
        lens = [L_of(row, 2 * tw + 1), L_of(row, tw + 1) + s - 1, L_of(row, tw), L_of(row, 3), 0, k - 1, nb, 2 * nb - 1, L_of(row, 2 * tw) + 1]
        reads = _placed(row, lens, rng)
        reads.append(_tract(unit, L_of(row, tw + 2), rng))
        return reads
    if row.reads == "capacity":                       # heads of ~24 kb: reads of at most 30 kb, so the two heads overlap
        reads = _placed(row, [30000, nb + 1, nb, nb - 1, 5000, k, 0, 29999], rng)
        reads.append(_tract(unit, nb + 777, rng, err=0.001))
        return reads
    if row.reads == "c255":                           # pure repeats: a window holds as many of one k-mer as fits
        n = L_of(row, 70)
        reads = [_tract(unit, n, rng), _tract(unit, n + 1, rng)[1:], _tract(unit, n, rng)[::-1], _tract(unit, L_of(row, 130) + s - 1, rng),
                 _tract(unit, n, rng, err=0.01), _rand(n, rng)[: n // 2] + _tract(unit, n, rng), _tract("AT", n, rng), _tract("A", n, rng)]
        return reads
    if row.reads == "heads":
        lens = [0, 1, k - 1, k, nb, 2 * nb - 1, nb + 1, 3000, 3001, 2 * nb + 2 * k + 50]
        reads = _placed(row, list(dict.fromkeys(x for x in lens if x >= 0)), rng, err=0.005)
        # pure tracts of exactly a k-mer, exactly a head, and two heads that overlap: counts wherever no_bp >= k
        return reads + [_tract(unit, k, rng), _tract(unit, nb, rng), _tract(unit, 2 * nb - 1, rng)[::-1].translate(COMP), _tract(unit, nb + k, rng) + _rand(500, rng)]
    if row.reads == "filter":                         # tracts of many lengths: step 1's best count spreads, and so do the lengths
        reads = []
        for i, (L, n) in enumerate([(6000, 900), (3000, 40), (5000, 400), (5000, 2000), (4000, 150), (7000, 0), (5000, 700), (2500, 2500), (5001, 90)]):
            seq = _tract(unit, n, rng, err=0.01) + _rand(L - n, rng)
            reads.append(seq if i % 2 == 0 else seq[::-1].translate(COMP))
        return reads
    if row.reads == "binseg":
        j, ms = row.jump, row.min_size
        counts = [1, 2, 3, 2 * ms - 1, 2 * ms, 2 * ms + 1, j, j + 1, j + ms, -(-ms // j) * j + ms - 1, -(-ms // j) * j + ms, 40, 200, tw + 3]
        lens = [L_of(row, n) + (i % s) for i, n in enumerate(dict.fromkeys(n for n in counts if n >= 1))]
        return _placed(row, lens, rng)
    if row.reads == "dirty":
        return dirty_reads(row)[0]
    raise ValueError(row.reads)


def tails_of(row, reads):
    """What a TAILS_IN row hands to set_tails: both tails over the reads, the skip bit on one of them."""
    t = (np.arange(len(reads)) % 2).astype(np.uint8)
    t[2] |= 2
    return t


# --------------------------------------------------------------------------------------------- oracle
_step1_cache: dict = {}
_win_cache: dict = {}


def step1_of(row, seq):
    key = (row.table, row.no_bp, seq)
    hit = _step1_cache.get(key)
    if hit is None:
        hit = _step1_cache[key] = occ.trc_counts(seq, row.patterns, row.no_bp)
    return hit


def windows_of(row, seq, tail):
    key = (row.table, row.W, row.s, row.t, row.M, tail, seq)
    hit = _win_cache.get(key)
    if hit is None:
        hit = _win_cache[key] = occ.window_counts(seq, "reverse" if tail else "forward", row.patterns, row.W, row.s, row.t, row.M)
    return hit


def decision(row, seq):
    """(tail, best count of that tail) as oracle.c's step 1 decides: forward only if strictly larger."""
    cs, ce = step1_of(row, seq)
    tail = 0 if max(cs) > max(ce) else 1
    return tail, (max(ce) if tail else max(cs))


FILTER_ANCHOR = 2             # the read of a filter row whose own best count / length the filter sits on


def filter_params(row, reads):
    """A filter row's parameters: min_count (or min_len) = the anchor read's best count (length) minus d.  d = 0 drops the read
    (both tests are strict), d = 1 keeps it."""
    what, d = row.filt
    seq = reads[FILTER_ANCHOR]
    if what == "count":
        return row.params(min_count=decision(row, seq)[1] - d, min_len=0)
    return row.params(min_len=len(seq) - d, min_count=0)


def params_of(row, reads):
    return filter_params(row, reads) if row.filt else row.params()


def resolve_with(sums, win_off, res, P, jump, min_size):
    """bkp with the RES_TIE reads handed to ruptures' float64 arithmetic (hiplib.resolve_ties, from downloaded S_w)."""
    b = res["bkp"].copy()
    for i in np.nonzero((res["flags"] & hiplib.RES_TIE) != 0)[0]:
        b[i] = hiplib.binseg_l2_float64(np.asarray(sums[win_off[i]:win_off[i + 1]], np.float64) / P, jump, min_size)
    return b


def check_scan(out, row, reads, prm, tails=None):
    """`out` = dict(results, win_off, c_start, c_end, sums, raw, bkp_resolved) of one scan of `reads` under `row` with `prm` (the
    emulation's or the GPU's); every field against oracle/oracle.c.  Returns the number of windows compared."""
    pats = row.patterns
    P = len(pats)
    res = out["results"]
    n = len(reads)
    assert len(res) == n
    step1 = bool(prm.flags & hiplib.F_STEP1)
    nw = np.array([hiplib.window_count(len(x), row.W, row.s, row.t, row.M) for x in reads], np.int64)
    want_off = np.concatenate([[0], np.cumsum(nw)])
    assert np.array_equal(out["win_off"], want_off), (row.id, "win_off")
    n_windows = 0
    saw_255 = False
    for i, seq in enumerate(reads):
        where = (row.id, i, len(seq))
        r = res[i]
        if step1:
            cs, ce = step1_of(row, seq)
            assert out["c_start"][i].tolist() == cs and out["c_end"][i].tolist() == ce, where + ("step-1 counts",)
            bs, be = max(cs), max(ce)
            assert (r["best_start"], r["best_end"]) == (bs, be), where
            assert (r["best_start_idx"], r["best_end_idx"]) == (cs.index(bs), ce.index(be)), where      # the first maximum
            tail = 0 if bs > be else 1
            passes = len(seq) > prm.min_len and (be if tail else bs) > prm.min_count
        else:
            tail, passes = int(tails[i]) & 1, not (int(tails[i]) & 2)
        assert r["tail"] == tail and r["pass"] == int(passes), where + ("tail / pass",)
        if not passes or not (prm.flags & hiplib.F_WINDOWS):
            assert r["n_win"] == 0 and r["bkp"] == -1, where
            # no kernel writes the windows of a read that does not pass: they are handed out as zeros (include/topsicle_hip.h)
            if "sums" in out:
                assert not out["sums"][want_off[i]:want_off[i + 1]].any(), where + ("S_w of a read that does not pass",)
            if row.raw and "raw" in out:
                assert not out["raw"][want_off[i]:want_off[i + 1]].any(), where + ("raw rows of a read that does not pass",)
            continue
        assert r["n_win"] == nw[i], where
        sums, raw = windows_of(row, seq, tail)
        lo, hi = want_off[i], want_off[i + 1]
        got = out["sums"][lo:hi]
        if not np.array_equal(got, sums):
            bad = int(np.nonzero(got != sums)[0][0])
            raise AssertionError(f"{where}: S_w differs first at window {bad} of {hi - lo}: got {got[bad]}, oracle {sums[bad]}")
        if row.raw:
            g = out["raw"][lo:hi]
            if not np.array_equal(g, raw):
                bad = np.argwhere(g != raw)[0]
                raise AssertionError(f"{where}: raw row differs first at window {bad[0]} pattern {bad[1]}: got {g[bad[0]]}, oracle {raw[bad[0]]}")
            saw_255 = saw_255 or bool((g == 255).any())
        n_windows += int(hi - lo)
        want = orc.binseg_l2_exact(sums, row.jump, row.min_size)
        assert r["bkp"] == (-1 if want is None else want), where + ("bkp", int(r["bkp"]), want)
        if r["flags"] & hiplib.RES_TIE:
            want64, _ = occ.binseg_l2_y(sums.astype(np.float64) / P, row.jump, row.min_size)          # (oracle.c's float64 Binseg)
            assert out["bkp_resolved"][i] == (-1 if want64 is None else want64), where + ("tie",)
    if row.want_255:
        assert saw_255, (row.id, "no raw byte holds 255")
    if row.filt:
        p = res["pass"].astype(bool)
        assert p.any() and (~p).any(), (row.id, "a filtering row must keep some reads and drop others")
        assert bool(p[FILTER_ANCHOR]) == (row.filt[1] == 1), (row.id, "pass flips on the anchor read's own count / length")
    return n_windows


# --------------------------------------------------------------------------------------------- the sanitizers' program
def digest(out, prm, P):
    """What tests/emu/emu_wide_main.cpp recomputes from its own scan: the decision and change point of every read, the step-1
    counts, S_w and raw bytes of the reads that passed (mod 2^64)."""
    res = out["results"]
    d = sum(m * int(res[f].astype(np.int64).sum()) for m, f in ((1, "pass"), (3, "tail"), (5, "n_win"), (7, "bkp"), (11, "best_start"), (13, "best_end")))
    if prm.flags & hiplib.F_STEP1:
        d += 23 * int(out["c_start"].astype(np.int64).sum()) + 29 * int(out["c_end"].astype(np.int64).sum())
    if prm.flags & hiplib.F_WINDOWS:
        keep = np.repeat(res["pass"].astype(bool), np.diff(out["win_off"]))
        d += 17 * int(out["sums"][keep].astype(np.int64).sum())
        if prm.flags & hiplib.F_STORE_RAW:
            d += 19 * int(out["raw"][keep].astype(np.int64).sum())
    return d % (1 << 64)


def dump_rows(path, rows, scan):
    """The file emu_wide_main.cpp replays.  Per row: int32 P, k, expected return code; P * k pattern letters; struct tps_params;
    uint64 digest of `scan(row, reads, prm, tails)` (0 for a refusal row); int64 n; n + 1 int64 offsets; the bases; n tail bytes."""
    with open(path, "wb") as f:
        for row in rows:
            reads = reads_of(row)
            prm = params_of(row, reads)
            tails = tails_of(row, reads) if prm.flags & hiplib.F_TAILS_IN else np.zeros(len(reads), np.uint8)
            bases, offsets = hiplib.pack_reads(reads)
            P = len(row.patterns)
            want = 0 if row.refuse else digest(scan(row, reads, prm, tails), prm, P)
            f.write(struct.pack("<iii", P, row.k, row.refuse) + "".join(row.patterns).encode() + bytes(prm) + struct.pack("<Qq", want, len(reads)))
            f.write(offsets.tobytes() + bases.tobytes() + tails.tobytes())
