"""The default sums-only tile (tile_lc_s, CD = 0) in the host emulation against the C oracle: the window phase in packed
16-bit pairs (home shape, q a multiple of 8) and the change-point candidates stored lane by lane from the lanes' own
prefixes.  S_w and the change point of every read must equal the oracle's; other window sizes (not the home shape),
every slide of the specialised kernels, reads that end inside a tile, small tiles and jumps other than 5 put the
candidates on every position inside a lane and on the first and last window of lanes and tiles."""
import numpy as np
import pytest

import emu_driver as emu
import oracle_c as occ
import topsicle_oracle as orc
from topsicle_amd import hiplib, synth

FLAGS = hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_TAILS_IN | hiplib.F_STORE_SUMS


def _reads(seed, n, lo, hi, motif="CCCTAA"):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        L = int(rng.integers(lo, hi))
        bases, offsets, _ = synth.make_reads(1, L, motif, int(rng.integers(1 << 30)), tract_min=L // 5, tract_max=L // 2)
        out.append(synth.split_reads(bases, offsets)[0])
    return out


def _check(pats, seqs, W, slide, jump, spans_pref=0):
    prm = hiplib.make_params(window=W, slide=slide, trimfirst=100, maxlen=20000, jump=jump, flags=FLAGS)
    out = emu.scan(pats, seqs, prm, tails=[0] * len(seqs), spans_pref=spans_pref)
    for i, seq in enumerate(seqs):
        want, _ = occ.window_counts(seq, "forward", pats, W, slide, 100, 20000)
        lo, hi = out["win_off"][i], out["win_off"][i + 1]
        got = out["sums"][lo:hi]
        assert np.array_equal(got, want), (W, slide, jump, i)
        r = out["results"][i]
        exact = orc.binseg_l2_exact(want, jump=jump)
        assert r["bkp"] == (-1 if exact is None else exact), (W, slide, jump, i)


def _counters():
    L = emu.lib()
    return L.emu_counter(3), L.emu_counter(7)


@pytest.mark.parametrize("slide", [5, 6, 7, 8])
@pytest.mark.parametrize("W", [100, 93, 101, 157])
def test_packed_tile_matches_oracle(slide, W):
    pats = orc.kmer_table("CCCTAA", 4)
    seqs = _reads(100 * slide + W, 4, 1500, 6000)
    _check(pats, seqs, W, slide, 5)


@pytest.mark.parametrize("jump", [4, 6, 7, 8, 9, 13])
def test_lane_candidates_other_jumps(jump):
    """jump != 5 moves the candidates to every window position inside a lane (jump >= 4: at most two per lane)."""
    pats = orc.kmer_table("CCCTAA", 4)
    seqs = _reads(jump, 3, 2000, 9000)
    _check(pats, seqs, 100, 6, jump)
    _check(pats, seqs, 93, 7, jump)


@pytest.mark.parametrize("jump", [1, 2, 3])
def test_small_jumps_keep_the_strided_pass(jump):
    pats = orc.kmer_table("CCCTAA", 4)
    seqs = _reads(50 + jump, 2, 1500, 4000)
    _check(pats, seqs, 100, 6, jump)


@pytest.mark.parametrize("spans_pref", [2, 3, 5])
def test_small_tiles_and_reads_ending_mid_tile(spans_pref):
    """Many tiles per read: candidates on the first and last window of tiles; every read length ends at another
    window of its last tile."""
    pats = orc.kmer_table("CCCTAA", 4)
    rng = np.random.default_rng(spans_pref)
    seqs = _reads(7 * spans_pref, 6, 700, 5000)
    seqs += [s[: int(rng.integers(400, len(s)))] for s in seqs[:3]]
    for jump in (4, 5, 8):
        _check(pats, seqs, 100, 6, jump, spans_pref=spans_pref)


def test_k5_table_and_the_new_paths_ran():
    """A k = 5 table (single lookups or the 16-bit pair table) next to the k = 4 pair table; the packed window phase and
    the lane candidates must have run in this module."""
    before = _counters()
    pats = orc.kmer_table("TTAGGG", 5)
    seqs = _reads(11, 3, 2000, 7000, motif="TTAGGG")
    _check(pats, seqs, 100, 6, 5)
    _check(orc.kmer_table("CCCTAA", 4), _reads(12, 2, 3000, 5000), 100, 6, 5)
    after = _counters()
    assert after[0] > before[0] and after[1] > before[1], (before, after)
