"""The change point of the fused kernels (csrc/tps_device.h binseg_from_lc) and the stores that feed it, path by path: which
finish ran is asserted from the emulation's counters (tests/emu_binseg_driver.py), every output goes against the C oracle
(kernel_matrix.check_scan: S_w, the boundary by exact integers, and for a flagged tie the float64 resolution).

  * `default`: a telomere with ONT-like errors and a random rest -- one candidate of the wave passes the prefilter, the one-lane
    finish takes it;
  * `close pair`: the two best candidates are neighbours (different lanes) 2.3e-5 apart, the third 1 % away: two lanes pass, the
    float64 stage of every lane and the wave reduction run, float64 separates them (no tie);
  * `same lane`: tract, filler, tract with palindromic window sums whose two best splits lie 64 candidates apart -- one lane
    holds both, the prefilter is `crowded` and the exact tournament decides (TPS_RES_TIE);
  * `tie`: test_binseg_integer_path's palindrome (the two splits in different lanes): an exact tie, flagged;
  * `constant`: every window sum the same -- every score is 0, every lane is close;
  * `nslot`: reads whose candidates fill 1, 4, 5, 8 and 9 slots per lane, the last slot holding 1 and 63 lanes;
  * `float64 D`: n T just above 2^31 (test_binseg_integer_path's bisected reads at window 255);
  * `stores`: jumps 4, 5, 8, 9 and 12 (one and two candidates per lane, first candidates that are not the lane's own), reads
    that end inside a tile, and the scratch block's capacity cut down to the longest read's candidates (lc_cap the binding
    bound: the last candidate is the block's last entry): the scratch block against prefix sums of the oracle's S_w, entry by
    entry, and nothing written behind the last candidate.

Emulation first, the `gpu` half with the same reads on the device (the finish that ran and the scratch block are only visible in
the emulation; the device half holds the outputs to the oracle and the tie flags)."""
from fractions import Fraction

import numpy as np
import pytest

import emu_binseg_driver as eb
import kernel_matrix as km
import oracle_c as occ
import test_binseg_integer_path as bi
import test_kernel_matrix as tkm
from topsicle_amd import hiplib

MOTIF = "CCCTAA"
ROW = km.Row("binseg_paths_W100", "p", kernel=km.kname("p", 6))
NSLOT_CANDS = (1, 63, 193, 255, 257, 319, 449, 511, 513, 575)      # 64 (nslot - 1) + 1 and + 63 for nslot = 1, 4, 5, 8, 9
STORE_JUMPS = (4, 5, 8, 9, 12)
UNWRITTEN = 0xBEEFBEEF


def _sums(row, seq):
    sums, _ = occ.window_counts(seq, "forward", row.patterns, row.W, row.s, row.t, row.M)
    return np.asarray(sums, np.int64)


def exact_scores(s, jump, min_size):
    """[(score as a Fraction, b)] of the admissible candidates, best first."""
    n, T = len(s), int(s.sum())
    L = np.concatenate([[0], np.cumsum(s)])
    out = []
    for b in range(jump, n, jump):
        if b >= min_size and n - b >= min_size:
            D = n * int(L[b]) - T * b
            out.append((Fraction(D * D, b * (n - b)), b))
    return sorted(out, reverse=True)


def default_read():
    rng = np.random.default_rng(11)
    return km._tract(MOTIF, 5000, rng, err=0.02) + km._rand(9000, rng)


def close_pair_read():
    rng = np.random.default_rng([77, 47])
    return km._tract(MOTIF, 3000 + 6 * 47, rng, err=0.08) + km._rand(5000, rng)


def same_lane_read():
    """Tract, 1 893 A, tract (palindromic window sums, 600 windows): the best split and its mirror image are 320 windows = 64
    candidates apart; 1 200 more A keep the end head empty and lie past maxlen."""
    body = (MOTIF * 100)[:ROW.t] + (MOTIF * 400)[:900] + "A" * 1893 + (MOTIF * 400)[2:2 + 901]
    return body + "A" * 1200, len(body)


def nslot_reads():
    rng = np.random.default_rng(5)
    out = []
    for nc in NSLOT_CANDS:
        n = ROW.jump * nc + 2                      # c_max = (n - min_size) / jump = nc, c_min = 1
        L = ROW.t + ROW.W + (n - 1) * ROW.s
        a = int(L * rng.uniform(0.3, 0.6))
        out.append((km._tract(MOTIF, a, rng, err=0.02) + km._rand(L - a, rng))[:L])
    return out


def store_reads(row):
    """Window counts 2 tw + 37 (ends inside the third tile), 1 020 (a multiple of jumps 4, 5 and 12), tw and 37."""
    rng = np.random.default_rng(9)
    out = []
    for n in (2 * row.tw + 37, 1020, row.tw, 37):
        L = row.t + row.W + (n - 1) * row.s + 3
        a = int(L * 0.4)
        out.append((km._tract(MOTIF, a, rng, err=0.03) + km._rand(L - a, rng))[:L])
    return out


def test_inputs_are_what_they_claim():
    s = _sums(ROW, close_pair_read())
    sc = exact_scores(s, ROW.jump, ROW.min_size)
    rel = lambda x: float((sc[0][0] - x) / sc[0][0])
    assert 1e-6 < rel(sc[1][0]) < 5e-5 and rel(sc[2][0]) > 1e-3, (rel(sc[1][0]), rel(sc[2][0]))
    assert abs(sc[0][1] - sc[1][1]) // ROW.jump % km.NT != 0, "different lanes"
    seq, M = same_lane_read()
    row = km.Row("x", "p", M=M, kernel=ROW.kernel)
    s = _sums(row, seq)
    sc = exact_scores(s, row.jump, row.min_size)
    assert km.tail_of(seq, row) == 0 and np.array_equal(s, s[::-1])
    assert sc[0][0] == sc[1][0] > sc[2][0] and abs(sc[0][1] - sc[1][1]) == km.NT * row.jump, sc[:3]
    for nc, seq in zip(NSLOT_CANDS, nslot_reads()):
        n = hiplib.window_count(len(seq), ROW.W, ROW.s, ROW.t, ROW.M)
        c_min, c_max = 1, min((n - ROW.min_size) // ROW.jump, (n - 1) // ROW.jump)
        assert c_max - c_min + 1 == nc, (nc, n)
    assert sorted({(nc + 63) // 64 for nc in NSLOT_CANDS}) == [1, 4, 5, 8, 9]
    assert {nc % 64 for nc in NSLOT_CANDS} == {1, 63}
    s = _sums(ROW, "A" * 2500)
    assert s.min() == s.max()


def _emu(row, reads):
    """(outputs checked against the oracle, the emulation counters' increments)."""
    with eb.counting() as cnt:
        out = tkm.emu_scan(row, reads, dirty=False)
    km.check_scan(out, row, reads, row.id)
    return out, cnt


def _tied(out):
    return (out["results"]["flags"] & hiplib.RES_TIE) != 0


def test_emulation_default_takes_the_one_lane_finish():
    reads = [default_read()]
    out, cnt = _emu(ROW, reads)
    assert (cnt[eb.ONE_LANE_FINISH], cnt[eb.WAVE_FINISH], cnt[eb.CROWDED], cnt[eb.EXACT_TOURNAMENTS], cnt[eb.F64_ROUTE]) == (1, 0, 0, 0, 0), cnt
    assert out["results"]["bkp"][0] > 0 and not _tied(out)[0]


def test_emulation_close_pair_in_two_lanes():
    reads = [close_pair_read()]
    out, cnt = _emu(ROW, reads)
    assert (cnt[eb.ONE_LANE_FINISH], cnt[eb.WAVE_FINISH], cnt[eb.CROWDED], cnt[eb.EXACT_TOURNAMENTS]) == (0, 1, 0, 0), cnt
    assert not _tied(out)[0]


def test_emulation_close_pair_in_one_lane_is_crowded():
    seq, M = same_lane_read()
    row = km.Row("binseg_paths_same_lane", "p", M=M, kernel=ROW.kernel)
    out, cnt = _emu(row, [seq])
    assert (cnt[eb.ONE_LANE_FINISH], cnt[eb.CROWDED], cnt[eb.EXACT_TOURNAMENTS]) == (0, 1, 1), cnt
    assert _tied(out)[0]


def test_emulation_exact_tie_still_flagged():
    seq, M = bi.tie_read(bi.DEFAULT)
    row = km.Row("binseg_paths_tie", "p", M=M, kernel=ROW.kernel)
    out, cnt = _emu(row, [seq, default_read(), seq])
    assert _tied(out).tolist() == [True, False, True]
    assert (cnt[eb.ONE_LANE_FINISH], cnt[eb.WAVE_FINISH], cnt[eb.EXACT_TOURNAMENTS]) == (1, 2, 2), cnt
    assert out["results"]["bkp"][0] == out["results"]["bkp"][2]


def test_emulation_constant_signal():
    reads = ["A" * 2500, default_read()]
    out, cnt = _emu(ROW, reads)
    assert (cnt[eb.ONE_LANE_FINISH], cnt[eb.WAVE_FINISH]) == (1, 1), cnt      # every score 0: every lane is close


def test_emulation_slot_counts():
    reads = nslot_reads()
    out, cnt = _emu(ROW, reads)
    assert cnt[eb.ONE_LANE_FINISH] + cnt[eb.WAVE_FINISH] == len(reads), cnt
    assert cnt[eb.F64_ROUTE] == 0, cnt


def test_emulation_float64_d_route():
    below, above = bi.bound_reads()
    out, cnt = _emu(bi.WIDE, [above])
    assert cnt[eb.F64_ROUTE] == 1 and cnt[eb.ONE_LANE_FINISH] + cnt[eb.WAVE_FINISH] == 1, cnt
    out, cnt = _emu(bi.WIDE, [below])
    assert cnt[eb.F64_ROUTE] == 0 and cnt[eb.ONE_LANE_FINISH] + cnt[eb.WAVE_FINISH] == 1, cnt


@pytest.mark.parametrize("jump", STORE_JUMPS)
def test_emulation_candidate_stores(jump):
    row = km.Row(f"binseg_paths_j{jump}", "p", jump=jump, kernel=ROW.kernel)
    reads = store_reads(row)
    out, cnt = _emu(row, reads)
    assert cnt[eb.LANE_CANDS] >= 3 + 3 + 1 + 1, cnt
    prm = row.params()
    prm.flags = hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS          # no step 1: forward tails
    before = eb.counters()
    n_max = 2 * row.tw + 37
    got = eb.scan_lc(row.patterns, reads, prm, lc_cap=n_max // jump + 1)      # the tightest capacity the longest read fits
    assert (eb.counters() - before)[eb.LANE_CANDS] >= 8
    assert got["lc_cap"] == n_max // jump + 1
    for i, seq in enumerate(reads):
        s = _sums(row, seq)
        n = len(s)
        assert np.array_equal(got["sums"][got["win_off"][i]:got["win_off"][i + 1]], s), (jump, i)
        pre = np.concatenate([[0], np.cumsum(s)])
        ncand = -(-n // jump)                       # candidates c with c jump < n, c = 0 included
        assert ncand <= got["lc_cap"]
        if i == 0 and n % jump:
            assert ncand == got["lc_cap"], "the longest read's last candidate is the block's last entry"
        want = pre[np.arange(ncand) * jump]
        lc = got["lc"][i]
        assert np.array_equal(lc[:ncand], want.astype(np.uint32)), (jump, i, "candidate sums")
        assert (lc[ncand:] == UNWRITTEN).all(), (jump, i, "a store behind the read's last candidate")
        assert got["results"]["bkp"][i] == km._bkp_exact(s, jump, row.min_size), (jump, i)


# ------------------------------------------------------------------------------------------------ the device half
@pytest.fixture(scope="module")
def sc():
    s = hiplib.HipScanner(0)
    yield s
    s.close()


def _gpu(sc, row, reads):
    from test_gpu_kernel_matrix import gpu_scan
    out, info = gpu_scan(sc, 0, row, reads, twice=True)
    assert info.split(" lds=")[0] == row.kernel, info
    km.check_scan(out, row, reads, row.id)
    return out


@pytest.mark.gpu
def test_gpu_default_and_close_pair(sc):
    out = _gpu(sc, ROW, [default_read(), close_pair_read(), "A" * 2500])
    assert not _tied(out)[:2].any() and (out["results"]["bkp"][:2] > 0).all()


@pytest.mark.gpu
def test_gpu_close_pair_in_one_lane(sc):
    seq, M = same_lane_read()
    out = _gpu(sc, km.Row("binseg_paths_same_lane", "p", M=M, kernel=ROW.kernel), [seq, default_read()])
    assert _tied(out).tolist() == [True, False]


@pytest.mark.gpu
def test_gpu_exact_tie_still_flagged(sc):
    seq, M = bi.tie_read(bi.DEFAULT)
    out = _gpu(sc, km.Row("binseg_paths_tie", "p", M=M, kernel=ROW.kernel), [seq, default_read(), seq])
    assert _tied(out).tolist() == [True, False, True]
    assert out["results"]["bkp"][0] == out["results"]["bkp"][2]


@pytest.mark.gpu
def test_gpu_slot_counts(sc):
    _gpu(sc, ROW, nslot_reads())


@pytest.mark.gpu
def test_gpu_float64_d_route(sc):
    below, above = bi.bound_reads()
    _gpu(sc, bi.WIDE, [above, below])


@pytest.mark.gpu
@pytest.mark.parametrize("jump", STORE_JUMPS)
def test_gpu_candidate_stores(sc, jump):
    row = km.Row(f"binseg_paths_j{jump}", "p", jump=jump, kernel=ROW.kernel)
    _gpu(sc, row, store_reads(row))
