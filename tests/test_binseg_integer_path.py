"""The change point's float32 prefilter computes D = n L_b - T b in 32-bit integers where n T < 2^31 and through float64 above
(csrc/tps_device.h binseg_from_lc): reads on both sides of that bound and an exact tie, every output against the C oracle
(kernel_matrix.check_scan: S_w, the boundary by exact integers, and for a flagged tie the float64 resolution).

  * `below` / `above`: a dense telomere at maxlen 20 000 and window 255 (3 275 windows of up to 252 matches: n T reaches 2.7e9),
    the tract's length bisected so that n T lies within 1 % under / over 2^31 -- the integer route's last and the float64
    route's first reads;
  * `default`: the same read at the default window (n T about 1.1e9: the integer route, the headline workload's shape);
  * `tie`: window sums that read the same from either end (tract, filler, tract: S == S[::-1], n a multiple of the jump), so the
    best split and its mirror image score EXACTLY the same: the later one wins and the read carries TPS_RES_TIE.

Emulation first, the `gpu` half on the device."""
import numpy as np
import pytest

import kernel_matrix as km
import oracle_c as occ
import test_kernel_matrix as tkm
from topsicle_amd import hiplib

BOUND = 1 << 31
MOTIF = "CCCTAA"
WIDE = km.Row("binseg_int_W255", "p", W=255, kernel=km.kname("p", 6))
DEFAULT = km.Row("binseg_int_W100", "p", kernel=km.kname("p", 6))
L_READ = 22000


def _sums(row, seq):
    sums, _ = occ.window_counts(seq, "forward", row.patterns, row.W, row.s, row.t, row.M)
    return np.asarray(sums, np.int64)


def _dense(a, rng_seed=5):
    """A read whose first `a` bases are the motif's tract, random after it (the same random bases for every a)."""
    rng = np.random.default_rng(rng_seed)
    tail = km._rand(L_READ, rng)
    return ((MOTIF * (a // 6 + 2))[:a] + tail)[:L_READ]


def _n_tot(row, seq):
    s = _sums(row, seq)
    return len(s) * int(s.sum())


def bound_reads():
    """(below, above): tract lengths bisected on n T against 2^31 at WIDE's window."""
    lo, hi = 2000, 20000
    assert _n_tot(WIDE, _dense(lo)) < BOUND < _n_tot(WIDE, _dense(hi))
    while hi - lo > 6:
        mid = (lo + hi) // 2 // 6 * 6
        if _n_tot(WIDE, _dense(mid)) < BOUND:
            lo = mid
        else:
            hi = mid
    return _dense(lo), _dense(hi)


def tie_read(row):
    """Tract, 603 A, tract: the window sums are a palindrome; 1 200 more A keep the end head empty (a forward tail) and lie
    past maxlen."""
    body = (MOTIF * 100)[:row.t] + (MOTIF * 400)[:900] + "A" * 603 + (MOTIF * 400)[2:2 + 901]
    return body + "A" * 1200, len(body)


def test_inputs_are_what_they_claim():
    below, above = bound_reads()
    nb, na = _n_tot(WIDE, below), _n_tot(WIDE, above)
    assert 0.99 * BOUND < nb < BOUND <= na < 1.01 * BOUND, (nb, na)
    assert _n_tot(DEFAULT, above) < 0.6 * BOUND
    for seq in (below, above):
        assert km.tail_of(seq, WIDE) == 0
    seq, M = tie_read(DEFAULT)
    row = km.Row("binseg_tie", "p", M=M, kernel=km.kname("p", 6))
    s = _sums(row, seq)
    assert km.tail_of(seq, row) == 0
    assert len(s) % row.jump == 0 and np.array_equal(s, s[::-1]) and s.min() < s.max()
    b = km._bkp_exact(s, row.jump, row.min_size)
    assert b > len(s) // 2, "the later of the two mirrored splits"


def _cases():
    below, above = bound_reads()
    tie, M = tie_read(DEFAULT)
    tie_row = km.Row("binseg_tie", "p", M=M, kernel=km.kname("p", 6))
    rng = np.random.default_rng(11)
    plain = [km._tract(MOTIF, 5000, rng, err=0.02) + km._rand(9000, rng)]
    return [(WIDE, [below, above] + plain, None), (DEFAULT, [above, below] + plain, None), (tie_row, [tie] + plain + [tie], (0, 2))]


def _check(out, row, reads, ties):
    km.check_scan(out, row, reads, row.id)
    res = out["results"]
    assert res["pass"].all() and (res["bkp"] >= 0).all()
    if ties:
        for i in ties:
            assert res["flags"][i] & hiplib.RES_TIE, (row.id, i, "an exact tie must be flagged")
        assert res["bkp"][ties[0]] == res["bkp"][ties[1]]


@pytest.mark.parametrize("case", range(3))
def test_emulation(case):
    row, reads, ties = _cases()[case]
    _check(tkm.emu_scan(row, reads, dirty=False), row, reads, ties)


@pytest.fixture(scope="module")
def sc():
    s = hiplib.HipScanner(0)
    yield s
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(3))
def test_gpu(sc, case):
    from test_gpu_kernel_matrix import gpu_scan
    row, reads, ties = _cases()[case]
    out, info = gpu_scan(sc, 0, row, reads, twice=True)
    assert info.split(" lds=")[0] == row.kernel, info
    _check(out, row, reads, ties)
