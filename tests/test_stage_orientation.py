"""Staging by orientation (csrc/tps_device.h scan_read: a forward tail's quads go to LDS as loaded, a reverse tail's are reversed
behind a wave-uniform branch; the lane's load offset is computed once per read): reads of BOTH tails on the edges of the
staging arithmetic, every output against the C oracle (kernel_matrix.check_scan).

  * the tile's first base at delta 0, 1, 62, 63 of its 64-base quad: for a forward tail delta = trimfirst % 64 (the rows), for a
    reverse tail delta = 63 - (L - 1 - trimfirst) % 64 (the read lengths);
  * the read's end on a quad edge and next to one (L % 64 in 0, 1, 63), which is where a reverse tail's first quad and a forward
    tail's last one sit;
  * non-ACGT letters in the scanned tail (first tile, second tile) and in either step-1 head, for both tails;
  * step-1 heads that are not a multiple of the packed count's 16-position chunk, and shorter than one chunk;
  * slide 8 (two quads per lane and tile) and the families that share scan_read (plain, 16-bit pair table, raw rows, self-overlap).

The first half runs the host emulation of the kernel source, the `gpu` half the same rows on the device, kernels asserted by name."""
import numpy as np
import pytest

import kernel_matrix as km
import test_kernel_matrix as tkm

DELTAS = (0, 1, 62, 63)


def _rows():
    R = []
    for t in (0, 1, 62, 63, 127):
        R.append(km.Row(f"orient_p_s6_t{t}", "p", t=t, kernel=km.kname("p", 6)))
    R.append(km.Row("orient_p_s6_nobp1007", "p", t=63, no_bp=1007, kernel=km.kname("p", 6)))
    R.append(km.Row("orient_p_s6_nobp12", "p", t=1, no_bp=12, kernel=km.kname("p", 6)))
    R.append(km.Row("orient_p_s8_t62", "p", s=8, t=62, kernel=km.kname("p", 8)))
    R.append(km.Row("orient_p_s5_t1", "p", s=5, t=1, no_bp=999, kernel=km.kname("p", 5)))
    R.append(km.Row("orient_plain_s7_t63", "plain", s=7, t=63, kernel=km.kname("plain", 7)))
    R.append(km.Row("orient_q_s6_t62", "q", t=62, no_bp=1001, kernel=km.kname("q", 6)))
    R.append(km.Row("orient_r_s6_t1", "r", t=1, kernel=km.kname("r", 6)))
    R.append(km.Row("orient_so_s6_t63", "so", t=63, no_bp=990, kernel=km.kname("so", 6)))
    R.append(km.Row("orient_generic_t62", "p", t=62, knobs={"force_generic": 1}, kernel=km.GENERIC))
    return R


ROWS = _rows()


def _anchor(row, L, tail, rng):
    """A read of L bases that takes `tail`: the motif's tract over its scanned end, random bases over the other."""
    n = min(L, max(row.no_bp + 40, int(L * 0.6)))
    fwd = km._tract(row.motif, n, rng, err=0.01) + km._rand(L - n, rng)
    return fwd if tail == 0 else fwd[::-1].translate(km.COMP)


def _put(seq, pos, ch="N"):
    return seq[:pos] + ch + seq[pos + 1:]


def orientation_reads(row):
    """(clean, dirty, notes): notes[i] = (tail, delta of tile 0, L % 64) of clean read i."""
    rng = np.random.default_rng([7, row.k, row.s, row.t, row.no_bp, row.W])
    s, t, W, nb = row.s, row.t, row.W, row.no_bp
    base = t + W + (2 * row.tw + 40) * s + 2 * nb            # three tiles, and the two heads apart
    clean, notes = [], []
    # forward tails: delta is the row's; the read's end on and next to a quad edge
    for end in (0, 1, 63, 17):
        L = (base // 64) * 64 + 64 + end
        clean.append(_anchor(row, L, 0, rng))
        notes.append((0, t % 64, L % 64))
    # reverse tails: every delta, by the length
    for d in DELTAS + (31,):
        L = base
        while 63 - ((L - 1 - t) % 64) != d:
            L += 1
        clean.append(_anchor(row, L, 1, rng))
        notes.append((1, d, L % 64))
    # ... and the read's end on and next to a quad edge
    for end in (0, 1, 63):
        L = (base // 64) * 64 + 128 + end
        clean.append(_anchor(row, L, 1, rng))
        notes.append((1, 63 - ((L - 1 - t) % 64), L % 64))
    # short reads: fewer bases than a head, one tile, one window
    for L in (nb - 1 if nb > 1 else 1, t + W + 5 * s, t + W - 1 + 64, 2 * nb - 3):
        for tail in (0, 1):
            if L > 0:
                clean.append(_anchor(row, L, tail, rng))
                notes.append((tail, None, L % 64))
    # dirty copies: one letter in the scanned tail's first and second tile, in the start head and in the end head
    dirty = []
    for tail, src in ((0, clean[0]), (1, clean[4]), (1, clean[7])):
        L = len(src)
        for x in (0, 63, 64, row.tw * s - 1, row.tw * s, row.tw * s + 65):
            dirty.append(_put(src, t + x if tail == 0 else L - 1 - t - x, "NRYn"[x % 4]))
        for pos in (0, min(nb, L) - 1, L - min(nb, L), L - 1, L - 1 - (min(nb, L) // 2)):
            dirty.append(_put(src, pos))
    return clean, dirty, notes


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_reads_are_on_their_edges(row):
    clean, dirty, notes = orientation_reads(row)
    tails = [km.tail_of(x, row) for x in clean]
    long_ = [i for i, n in enumerate(notes) if n[1] is not None]
    assert [tails[i] for i in long_] == [notes[i][0] for i in long_]
    assert {notes[i][1] for i in long_ if notes[i][0] == 1} >= set(DELTAS)
    assert {notes[i][1] for i in long_ if notes[i][0] == 0} == {row.t % 64}
    for tail in (0, 1):
        assert {notes[i][2] for i in long_ if notes[i][0] == tail} >= {0, 1, 63}
    assert all(set(x) - set("ACGT") for x in dirty)
    assert {km.tail_of(x, row) for x in dirty} == {0, 1}


def test_rows_cover_every_delta_of_a_forward_tail():
    assert {r.t % 64 for r in ROWS if r.kernel == km.kname("p", 6)} >= set(DELTAS)
    assert any(r.no_bp % 16 and r.no_bp > 16 for r in ROWS) and any(r.no_bp < 16 for r in ROWS)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_emulation(row):
    clean, dirty, _ = orientation_reads(row)
    a = tkm.emu_scan(row, clean, dirty=False)
    km.check_scan(a, row, clean, "clean")
    lo = len(dirty) // 2
    batch = dirty[:lo] + clean + dirty[lo:]
    b = tkm.emu_scan(row, batch, dirty=True)
    km.check_scan(b, row, batch, "dirty")
    km.same_outputs(a, b, np.arange(len(clean)), np.arange(lo, lo + len(clean)), row.id + " clean reads in a dirty batch")


@pytest.fixture(scope="module")
def sc():
    from topsicle_amd import hiplib
    s = hiplib.HipScanner(0)
    yield s
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_gpu(sc, row):
    from test_gpu_kernel_matrix import gpu_scan
    clean, dirty, _ = orientation_reads(row)
    a, info = gpu_scan(sc, 0, row, clean, twice=True)
    assert info.split(" lds=")[0] == row.expected(False), info
    km.check_scan(a, row, clean, "clean")
    lo = len(dirty) // 2
    batch = dirty[:lo] + clean + dirty[lo:]
    b, info = gpu_scan(sc, 1, row, batch, twice=True)
    assert info.split(" lds=")[0] == row.expected(True), info
    km.check_scan(b, row, batch, "dirty")
    km.same_outputs(a, b, np.arange(len(clean)), np.arange(lo, lo + len(clean)), row.id + " clean reads in a dirty batch")
