"""tps_followers_kernel_wide on the MI355X, everything through the C ABI (tps_batch_kmer_followers_wide): the checks of
tests/test_wide_overview.py (tests/wide_overview_checks.py) on the real kernel, 4000 x 15 kb reads of a 23-letter motif with the
kernel's own invariants, and overview_plot end to end on long motifs."""
import ctypes as C

import numpy as np
import pytest

import record_wide_overview as rec
import topsicle_oracle as orc
import wide_overview_checks as chk
from topsicle_amd import allsteps, hiplib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture()
def engine():
    e = hiplib.HipScanner(0)
    allsteps.set_engine(e)
    yield e
    allsteps.set_engine(None)
    e.close()


@pytest.mark.parametrize("name", list(rec.RUNS))
def test_rows_equal_reference_on_gpu(name, gold_dir, tmp_path, engine):
    chk.check_fixture(name, gold_dir, tmp_path, engine)


@pytest.mark.parametrize("seed", range(14))
def test_followers_wide_random_vs_oracle_on_gpu(engine, seed):
    chk.check_random_reads_against_oracle(engine, seed)


def test_wide_entry_equals_narrow_entry_on_gpu(engine):
    chk.check_old_against_new(engine)


def test_error_paths_are_loud_on_gpu(engine):
    chk.check_error_paths(engine)
    # the C ABI itself: a histogram with more than 8 following letters is TPS_E_CAPACITY, a narrow table TPS_E_PATTERN; the
    # context answers the next call as if nothing had happened
    engine.set_patterns_wide(allsteps.patterns_to_search(rec.M23, 6))
    engine.upload(0, *hiplib.pack_reads([rec.M23 * 100]))
    picks = np.zeros((1, 2, 23, 60), np.uint32)
    hist = np.zeros(8, np.int64)
    args = (engine._h, 0, 23, 17, 100, 2000, 0, picks.ctypes.data_as(C.c_void_p), picks.size)
    assert engine.lib.tps_batch_kmer_followers_wide(*args, hist.ctypes.data_as(C.c_void_p), hist.size) == -5
    assert b"follow" in engine.lib.tps_last_error()
    assert engine.lib.tps_batch_kmer_followers_wide(*args, None, 0) == 0 and picks.any()
    # ... and what HipScanner.kmer_followers_wide turns away before the library sees it: (n_fwd, follow, lo, hi) -> the library's own answer
    pp, pn = picks.ctypes.data_as(C.c_void_p), picks.size
    for n_fwd, follow, lo, hi, want in ((0, 2, 100, 2000, -3), (33, 2, 100, 2000, -3), (24, 2, 100, 2000, -3), (23, -1, 100, 2000, -3),
                                        (23, 2, 500, 500, -5), (23, 2, 2000, 100, -5), (23, 2, -1, 2000, -5), (23, 2, 0, 4097, -5)):
        assert engine.lib.tps_batch_kmer_followers_wide(engine._h, 0, n_fwd, follow, lo, hi, 0, pp, pn, None, 0) == want, (n_fwd, follow, lo, hi)
        assert engine.lib.tps_last_error()
    assert engine.lib.tps_batch_kmer_followers_wide(engine._h, 0, 23, 17, 100, 2000, 0, pp, pn - 1, None, 0) == -3       # picks of the wrong size
    assert engine.lib.tps_batch_kmer_followers_wide(engine._h, 0, 23, 2, 100, 2000, 0, pp, pn, hist.ctypes.data_as(C.c_void_p), hist.size) == -3   # hist of the wrong size
    assert engine.lib.tps_batch_kmer_followers_wide(*args, None, 0) == 0
    engine.set_patterns(allsteps.patterns_to_search("CCCTAA", 4))
    assert engine.lib.tps_batch_kmer_followers_wide(*args, None, 0) == -4


def test_followers_wide_batch_properties_on_gpu(engine):
    """4000 config-shaped reads of the 23-letter motif: the histogram equals the picks' count, the reverse-complemented batch
    swaps the two strands, and single reads equal the oracle's rows."""
    motif, k = rec.M23, 21
    n_fwd, follow = len(motif), 2
    engine.set_patterns_wide(allsteps.patterns_to_search(motif, k))
    n, L = 4000, 15000
    bases, offsets, _ = synth.make_reads(n, L, motif, seed=5, errors=synth.HIFI)
    engine.upload(1, bases, offsets)
    picks, hist = engine.kmer_followers_wide(1, n_fwd, follow, 100, 2000, 9000)
    total = int(np.unpackbits(picks.view(np.uint8)).sum())
    print(f"{total} picks, histogram sum {int(hist.sum())}")
    assert total == int(hist.sum()) > n * 20
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    rc = comp[bases.reshape(n, L)[:, ::-1]].reshape(-1)
    engine.upload(2, rc, offsets)
    picks_rc, hist_rc = engine.kmer_followers_wide(2, n_fwd, follow, 100, 2000, 9000)
    assert np.array_equal(picks[:, 0], picks_rc[:, 1]) and np.array_equal(picks[:, 1], picks_rc[:, 0])
    assert np.array_equal(hist[0], hist_rc[1]) and np.array_equal(hist[1], hist_rc[0])
    for i in (0, 77, 3999):
        seq = bytes(bases[offsets[i]:offsets[i + 1]]).decode()
        for strand, rows in enumerate(orc.kmer_followers(seq, motif, k)):
            for j, p in enumerate(orc.kmers_of_repeat(motif, k)):
                bits = np.unpackbits(picks[i, strand, j].view(np.uint8), bitorder="little")
                assert np.flatnonzero(bits).tolist() == [pos for q, _m, pos in rows if q == p]
    # seventeen followers (k = 6): no histogram, the same invariants on the picks
    engine.set_patterns_wide(allsteps.patterns_to_search(motif, 6))
    p6, none = engine.kmer_followers_wide(1, n_fwd, 17, 100, 2000, 9000, want_hist=False)
    p6_rc, _ = engine.kmer_followers_wide(2, n_fwd, 17, 100, 2000, 9000, want_hist=False)
    assert none is None and p6.any() and np.array_equal(p6[:, 0], p6_rc[:, 1]) and np.array_equal(p6[:, 1], p6_rc[:, 0])


@pytest.mark.parametrize("motif", list(chk.E2E_MOTIFS))
def test_overview_driver_long_motif_on_gpu(tmp_path, motif):
    chk.check_overview_end_to_end(tmp_path, chk.E2E_MOTIFS[motif], None)
