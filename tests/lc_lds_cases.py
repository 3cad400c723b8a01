"""The batches of tests/test_lc_lds_emulation.py and tests/test_gpu_lc_lds.py: CCCTAA at k = 4, window 100, slide 6 (the pair-table
kernel tps_scan_kernel_s6p), the shapes at which resident candidate sums (ScanArgs::lc_lds) can go wrong.  A tile is 494 windows; a
read of n windows is trimfirst + 100 + 6 (n - 1) bases; the region of slide 6 holds 736 entries and a scan needs lc_cap + 2 =
max n / jump + 4 of them; unwrapping is exact while (c_min + 64) jump (96 + 12) < 65 536, i.e. up to jump 9 at min_size 2."""
import dataclasses

import numpy as np

import kernel_matrix as km

MOTIF = "CCCTAA"
KERNEL = km.kname("p", 6)
ENTRIES = 736                       # 2 * (576 - 208) 16-bit entries behind the staged bases of a slide-6 tile
TILE_EDGES = (493, 494, 495, 496, 988, 989, 2467, 3301)


def length(n, row):
    return row.t + row.W + row.s * (n - 1)


def read_n(n, row, rng, frac=0.4, err=0.03, reverse=False):
    """A read of n windows: a telomere tract with errors over `frac` of it, then random sequence (reverse: the tract at the end)."""
    L = length(n, row)
    a = int(L * frac)
    seq = (km._tract(MOTIF, a, rng, err=err) + km._rand(L - a, rng))[:L]
    return seq[::-1].translate(str.maketrans("ACGT", "TGCA")) if reverse else seq


@dataclasses.dataclass
class Case:
    id: str
    row: km.Row
    reads: list
    resident: bool              # what the plan must decide for this batch
    dirty: bool = False         # the batch holds non-ACGT letters
    ties: tuple = ()            # reads the exact tournament must decide (TPS_RES_TIE)


def _row(tag, **kw):
    return km.Row("lc_lds_" + tag, "p", kernel=KERNEL, **kw)


def cases():
    out = []
    rng = np.random.default_rng(23)
    row = _row("edges")
    # tile boundaries, the longest read the reference's default maxlengthtelo allows among short ones
    out.append(Case("tile_edges", row, [read_n(n, row, rng) for n in TILE_EDGES] + [read_n(37, row, rng)], True))
    for jump in (4, 5, 8, 9):
        r = _row(f"j{jump}", jump=jump)
        out.append(Case(f"jump{jump}", r, [read_n(n, r, rng, frac=f) for n, f in ((495, 0.3), (989, 0.6), (2467, 0.2), (61, 0.5))], True))
    r = _row("j3", jump=3)
    out.append(Case("jump3_off_chip", r, [read_n(n, r, rng) for n in (495, 989)], False))
    r = _row("j10", jump=10)
    out.append(Case("jump10_wrap_bound_fails", r, [read_n(n, r, rng) for n in (495, 989)], False))
    # lc_cap + 2 = n / 4 + 4: 736 at n = 2 931, 737 at n = 2 932
    r = _row("cap", jump=4)
    out.append(Case("capacity_exact", r, [read_n(2931, r, rng), read_n(495, r, rng)], True))
    out.append(Case("capacity_one_over", r, [read_n(2932, r, rng), read_n(495, r, rng)], False))
    # telomere from end to end: the prefix sums pass 2^16 five times (with errors: a change point somewhere; without: a constant signal)
    row = _row("wrap")
    out.append(Case("wrap_around", row, [km._tract(MOTIF, length(3301, row), rng, err=0.05), (MOTIF * 3400)[:length(3301, row)]], True, ties=(1,)))
    # no match at all: every S_w = P, every score 0 -- the exact tournament decides, behind the moved fence
    out.append(Case("constant_signal", row, ["A" * 2500, read_n(989, row, rng), "A" * length(3301, row)], True, ties=(0, 2)))
    # both tails, a read shorter than one window, one whose window count admits no change point
    out.append(Case("tails_and_short", row, [read_n(989, row, rng), read_n(989, row, rng, reverse=True), read_n(496, row, rng, reverse=True),
                                             km._rand(150, rng), read_n(3, row, rng), read_n(1, row, rng)], True))
    # step 1 refuses some reads (a filtering row: min_len 3 000, the cutoff's min_count)
    r = _row("filt", filt=True)
    out.append(Case("step1_filter", r, [read_n(989, r, rng), km._rand(6000, rng), read_n(300, r, rng), read_n(2467, r, rng, reverse=True)], True))
    # one read with Ns: the INV tile wherever a tile of it holds one
    dirty = list(read_n(1200, row, rng))
    for p in (150, 151, 3000, 5999, 6000, 7100):
        dirty[p] = "N"
    out.append(Case("with_N", row, [read_n(495, row, rng), "".join(dirty), read_n(989, row, rng)], True, dirty=True))
    return out


CASES = cases()
