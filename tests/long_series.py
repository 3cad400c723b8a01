"""Shared rows and reads of the long-series tests (tests/test_long_series.py on the host emulation, tests/test_gpu_long_series.py
on the MI355X).  Not collected by pytest: no test_ prefix.  Built like tests/kernel_matrix.py, whose Row, checkers and oracle
cache it uses.

"Long" means more windows per read than any other test scans: every row has maxlen M = 62 000 (`--maxlengthtelo` raised), which
at window 100 and slide 6 is 10 301 windows or 21 fused tiles per read, against 3 301 windows / 7 tiles at the default 20 000.

ROWS: one row per kernel family at slide 6, one family each at slides 5, 7 and 8, the default kernels' slides 3 and 12, the generic
kernel (the knob, and a slide without a fused kernel), two filtering rows; WIDE_ROWS: a 16-letter and a 23-letter motif through
tps_scan_kernel_wide.  The kernel every row must launch is the one it launches at M = 20 000.

`reads_of(row)` builds a handful of reads (the batch stays under 1 MB): window counts 1, 8, 7 tw, 7 tw + 1, 8 tw - 1 (the first
tiles no test reached), the two counts on either side of the change point's prefilter limit (`prefilter_edge`: derived from
binseg_from_lc's c_max - c_min < 16 x 64), the count at M, a read of 2 M bases; tracts at the start, at the end, at both ends and
absent, on both strands, with ONT-like errors; a pure repeat of M bases (the largest T), a read whose window sums are a palindrome
over more than 6 145 windows (its two best splits tie exactly: the exact tournament on a long series), and a long read without
a telomere (it fails a filtering row's cutoff).  The dirty copies carry one non-ACGT letter each in a window of a tile past the
14th: on a window's first base, on its last base, on the tile's first window's first base, in the coordinates of the copy's own
tail.  With M = 62 000 the scanned string ends at position 61 899, so nothing inside it lies beyond 65 535; the reverse tail's
copies have their letters at READ positions beyond 65 535, and the row DEEP (M = 140 000, a few reads only) puts them at
scanned-string positions beyond 65 535 as well.

`stride_batches(row)` builds the two batches of a strided row (slides 10 and 15: every 2nd / 3rd window of the slide-5 kernels):
one whose longest read has exactly 6 144 windows at the requested slide -- the largest series tps_stride_kernel keeps in LDS --
and one with 6 145, the first it reads back from HBM.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import kernel_matrix as km
import oracle_c as occ
import topsicle_oracle as orc
import wide_cases
import wide_path_rows as wp
from topsicle_amd import hiplib

M_LONG = 62000
NT = km.NT
LCV = 16                       # binseg_from_lc: the prefilter holds at most LCV candidates per lane
STRIDE_LDS_MAX = 6144          # do_scan_strided: s16_dw <= 3072 dwords of 16-bit sums per wave
COMP = km.COMP


def _rows():
    R = []
    for fam in ("plain", "p", "r", "so", "sol", "sor", "sorh", "q"):
        R.append(km.Row(f"long_{fam}_s6", fam, M=M_LONG, kernel=km.kname(fam, 6)))
    R.append(km.Row("long_sixteen_s6", "sixteen", M=M_LONG, kernel=km.kname("so", 6), kernel_dirty=km.GENERIC))
    for fam, s in (("so", 5), ("q", 7), ("sor", 8)):
        R.append(km.Row(f"long_{fam}_s{s}", fam, s=s, M=M_LONG, kernel=km.kname(fam, s)))
    R.append(km.Row("long_p_s3", "p", s=3, M=M_LONG, kernel=km.kname("p", 3)))
    R.append(km.Row("long_p_s12", "p", s=12, W=110, M=M_LONG, kernel=km.kname("p", 12)))
    R.append(km.Row("long_p_s6_force_generic", "p", M=M_LONG, knobs={"force_generic": 1}, kernel=km.GENERIC))
    R.append(km.Row("long_p_s13", "p", s=13, W=120, M=M_LONG, kernel=km.GENERIC))
    for fam in ("p", "sor"):
        R.append(km.Row(f"long_{fam}_s6_filter", fam, M=M_LONG, filt=True, kernel=km.kname(fam, 6)))
    return R


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
# letters at scanned-string positions beyond 65 535 need a longer scanned string: the anchors and their dirty copies only
DEEP = km.Row("long_p_s6_M140000", "p", M=140000, kernel=km.kname("p", 6))


@dataclasses.dataclass
class WideRow(wp.Row):
    """A wide_path_rows.Row with a table of its own (wide_path_rows.TABLES stays what its tests say it is)."""
    motif: str = ""
    wk: int = 0

    @property
    def patterns(self):
        return orc.kmer_table(self.motif, self.wk)


WIDE_ROWS = [WideRow("long_wide_m16k16", "long_m16k16", M=M_LONG, unit=wide_cases.MOTIFS[16], motif=wide_cases.MOTIFS[16], wk=16),
             WideRow("long_wide_m23k21", "long_m23k21", M=M_LONG, unit=wide_cases.MOTIFS[23], motif=wide_cases.MOTIFS[23], wk=21)]

# strided rows: (family, slide, base slide, every m-th); filtering rows, so that one read of each batch does not pass
STRIDED = [("r", 10, 5, 2), ("so", 10, 5, 2), ("r", 15, 5, 3), ("so", 15, 5, 3)]


def stride_row(fam, slide):
    L = L_of_shape(100, 100, slide, STRIDE_LDS_MAX + 1)
    return km.Row(f"long_{fam}_s{slide}_strided", fam, s=slide, M=L + slide, filt=True)


def stride_name(fam, base, m):
    return km.kname(fam, base) + {2: " every 2nd window", 3: " every 3rd window"}[m]


# --------------------------------------------------------------------------------------------- shapes
def L_of_shape(t, W, s, n):
    return t + W + (n - 1) * s


def L_of(row, n):
    """The shortest read with n >= 1 windows (kernel_matrix.edge_lengths)."""
    return L_of_shape(row.t, row.W, row.s, n)


def cand_range(n, jump, min_size):
    """(c_min, c_max) of binseg_from_lc (csrc/tps_device.h): the admissible candidates b = c jump of a series of n windows."""
    ncand = (n - 1) // jump
    c_min = max(-(-min_size // jump), 1)
    c_max = min((n - min_size) // jump, ncand)
    return c_min, c_max


def prefilter_on(n, jump, min_size):
    c_min, c_max = cand_range(n, jump, min_size)
    return c_max - c_min < LCV * NT


def prefilter_edge(jump, min_size):
    """(n_on, n_off): the largest window count whose candidates the prefilter still holds, and the next one up."""
    n = jump * LCV * NT
    while prefilter_on(n, jump, min_size):
        n += 1
    return n - 1, n


def nwin(row, seq):
    return hiplib.window_count(len(seq), row.W, row.s, row.t, row.M)


# --------------------------------------------------------------------------------------------- reads
def palindrome_read(row, n=None):
    """A read whose window sums read the same from either end over n windows (n a multiple of the jump, more than 6 145): P, the
    trimmed t bases of tract; then tract [0, a), gap, tract, filler, and the same mirrored, every tract segment whole motifs --
    a segment [x, y) of matching positions and its image [E - y, E - x) under the mirror of the scanned string give window w and
    window n - 1 - w the same count whatever the motif's phase, because the table holds every rotation.  The gap at 900 .. 1100
    (and its image) keeps the end head below the start head, which has P instead: a forward tail, strictly.  The filler letter is
    the first that forms no pattern across a junction, checked against the oracle.  Returns the read, or None where M holds fewer
    than n windows or no letter works."""
    motif, k, t, W, s = row.motif, row.k, row.t, row.W, row.s
    m = len(motif)
    if n is None:
        n = (STRIDE_LDS_MAX + 2 + row.jump - 1) // row.jump * row.jump
    E = (n - 1) * s + W - 1                       # window n - 1 reads up to character E - 1; one more base makes it count (window_count)
    a = 900 // m * m
    g1 = 1100
    b = (E // 2 - 3000 - g1) // m * m             # the long segment [g1, g1 + b)
    if L_of(row, n) + 1 > row.M:                  # (slides 12 and 13: M holds fewer windows)
        return None
    assert g1 + b < E // 2
    pre = (motif * (t // m + 2))[-t:] if t else ""
    for f in "TAGC":
        body = [f] * E
        for lo, ln in ((0, a), (g1, b)):
            seg = (motif * (ln // m))
            body[lo:lo + ln] = seg
            body[E - lo - ln:E - lo] = seg
        seq = pre + "".join(body) + f
        if km.tail_of(seq, row) != 0:
            continue
        sums, _ = occ.window_counts(seq, "forward", row.patterns, W, s, t, row.M)
        sums = np.asarray(sums)
        if len(sums) == n and np.array_equal(sums, sums[::-1]) and sums.max() > sums.min():
            return seq
    return None


def _placed(row, L, mode, rc, rng, frac=None):
    """A read of L bases: mode 0 the telomere at the start (the motif's tract: a forward tail), 1 at the end (its reverse
    complement: a reverse tail), 2 at both ends (equal heads), 3 none; rc: the whole read on the other strand."""
    motif, k, nb = row.motif, row.k, row.no_bp
    if mode == 2 and L >= 2 * nb + 2 * k:
        tr = km._tract(motif, nb + k, rng)
        seq = tr + km._rand(L - 2 * len(tr), rng) + tr[::-1].translate(COMP)
    else:
        n = int(L * (rng.uniform(0.2, 0.7) if frac is None else frac)) if mode < 3 else 0
        seq = (km._tract(motif, n, rng, err=0.02) + km._rand(L - n, rng))[:L]
        if mode == 1:
            seq = seq[::-1].translate(COMP)
    return seq[::-1].translate(COMP) if rc else seq


def _rng(row, salt):
    return np.random.default_rng([salt, row.k, row.W, row.s, row.t, row.M, row.no_bp, sum(map(ord, row.motif))])


def _anchors(row, rng, tiles, L):
    """Two reads whose tail step 1 cannot miss: a tract over the windows of `tiles` tiles and a random rest up to L bases (the
    forward tail), and its reverse complement (the reverse tail)."""
    n = row.t + row.W + tiles * row.tw * row.s + 8 * row.s
    fwd = km._tract(row.motif, n, rng, err=0.01) + km._rand(L - n, rng)
    assert L - n >= row.no_bp + 8 * row.s
    return [fwd, fwd[::-1].translate(COMP)]


def _dirty(row, anchors, tile):
    """Copies of the anchors with one non-ACGT letter: on the first and the last base of window `tile` tw + 3, and on the first base
    of tile `tile`'s first window, in the coordinates of the anchor's own tail (a window holds W - 1 characters)."""
    dirty, marks = [], []
    letters = "NRn-YKWS"
    tw, s, W, t = row.tw, row.s, row.W, row.t
    for tail, a in enumerate(anchors):
        L = len(a)
        w = tile * tw + 3
        for kind, x in ((f"window {w}'s first base", w * s), (f"window {w}'s last base", w * s + W - 2),
                        (f"tile {tile}'s first window's first base", tile * tw * s)):
            assert x <= (nwin(row, a) - 1) * s + W - 2
            marks.append(km.Mark(kind, tail, t + x if tail == 0 else L - 1 - t - x, x))
        if tail == 1:            # near the scanned string's start the reverse tail's letter sits at the read's far end
            marks.append(km.Mark("window 3's first base", tail, L - 1 - t - 3 * s, 3 * s))
    for i, mk in enumerate(marks):
        a = anchors[mk.tail]
        dirty.append(a[:mk.pos] + letters[i % len(letters)] + a[mk.pos + 1:])
    return dirty, marks


_cache: dict = {}
DIRTY_TILE = 15               # the dirty letters' tile: past the 14th (slide 8: the 15th, M's last whole tile; slides 12 and 13: M holds 10 and 9 tiles)


def dirty_tile(row):
    n_M = hiplib.window_count(row.M, row.W, row.s, row.t, row.M)
    return min(DIRTY_TILE, n_M // row.tw - 1)


def reads_of(row):
    """(clean reads, dirty copies, marks, names): `names` maps "n_on", "n_off", "at_M", "two_M", "pure", "palindrome", "no_telomere"
    to indices of `clean`.  Deterministic in the row's table and shape."""
    key = (row.motif, row.k, row.W, row.s, row.t, row.M, row.no_bp, row.jump, row.min_size, row.tw)
    if key in _cache:
        return _cache[key]
    rng = _rng(row, 1)
    tw = row.tw
    n_on, n_off = prefilter_edge(row.jump, row.min_size)
    n_M = hiplib.window_count(row.M, row.W, row.s, row.t, row.M)
    clean, names = [], {}
    # (window count, tract placement as in _placed, other strand, name, tract fraction); the prefilter's edge reads are dense (19 of 20
    # bases in the tract): n T >= 2^31 with the prefilter still on
    plan = [(1, 0, False, None, None), (8, 1, False, None, None), (7 * tw, 2, True, None, None), (7 * tw + 1, 3, True, None, None),
            (8 * tw - 1, 0, True, None, None), (n_on, 1, False, "n_on", 0.95), (n_off, 0, False, "n_off", 0.95), (n_M, 2, False, "at_M", None)]
    for i, (n, mode, rc, name, frac) in enumerate(plan):
        L = row.M if n == n_M else L_of(row, n) + i % row.s
        clean.append(_placed(row, L, mode, rc, rng, frac))
        if name:
            names[name] = i
    names["two_M"] = len(clean)
    clean.append(_placed(row, 2 * row.M, 1, True, rng, 0.6))
    names["pure"] = len(clean)
    clean.append(km._tract(row.motif, row.M, rng))
    pal = palindrome_read(row)
    if pal is not None:
        names["palindrome"] = len(clean)
        clean.append(pal)
    names["no_telomere"] = len(clean)
    clean.append(km._rand(40000, rng))
    tile = dirty_tile(row)
    anchors = _anchors(row, rng, tile + 1, max(L_of(row, (tile + 1) * tw) + 2 * row.no_bp, 70000))     # (70 000: read positions beyond 65 535)
    dirty, marks = _dirty(row, anchors, tile)
    hit = _cache[key] = (clean, anchors + dirty, [None, None] + marks, names)
    return hit


def deep_reads():
    """DEEP's reads: anchors of 100 000 bases and their dirty copies, the letters in tile 23 -- scanned-string positions beyond 65 535."""
    key = "deep"
    if key not in _cache:
        row = DEEP
        rng = _rng(row, 2)
        tile = 65536 // (row.tw * row.s) + 1
        anchors = _anchors(row, rng, tile + 1, 100000)
        dirty, marks = _dirty(row, anchors, tile)
        _cache[key] = ([km._rand(900, rng)], anchors + dirty, [None, None] + marks, {})
    return _cache[key]


def batches(row):
    """(clean batch, dirty batch): the dirty batch is the anchors, their dirty copies and the clean batch's two shortest reads."""
    clean, dirty, _, _ = deep_reads() if row is DEEP else reads_of(row)
    return clean, dirty[: len(dirty) // 2] + clean[:2] + dirty[len(dirty) // 2:]


def short_batch(row, seed=3):
    """Reads under 3 000 bases (slot reuse: short batch, long batch, short batch)."""
    rng = _rng(row, seed)
    return [_placed(row, int(L), i % 4, i % 2 == 1, rng) for i, L in enumerate(rng.integers(300, 3000, 24))]


def stride_batches(row):
    """(batch whose longest read has 6 144 windows at row.s, batch whose longest has 6 145): with them reads of 0, 1 and 8 windows,
    a medium read, and a long read without a telomere (it does not pass the row's cutoff and is shorter than the longest)."""
    key = ("stride", row.motif, row.k, row.s, row.M)
    if key not in _cache:
        rng = _rng(row, 4)
        common = [_placed(row, L_of(row, 1) - 1, 0, False, rng), _placed(row, L_of(row, 1), 1, False, rng), _placed(row, L_of(row, 8) + 3, 0, True, rng),
                  km._rand(L_of(row, 3000), rng), _placed(row, L_of(row, 1500) + 1, 1, True, rng)]
        out = []
        for n, rc in ((STRIDE_LDS_MAX, False), (STRIDE_LDS_MAX + 1, True)):
            out.append(common[:3] + [_placed(row, L_of(row, n) + row.s - 1, 0, rc, rng, 0.55)] + common[3:])
        _cache[key] = tuple(out)
    return _cache[key]


# --------------------------------------------------------------------------------------------- wide rows
def wide_reads(row):
    """(clean batch, dirty batch) of a wide row: the same reads on the wide kernel's tiles (tw = 640 windows of 4 096 positions)."""
    return batches(row)
