"""Resident candidate sums of the default kernels (ScanArgs::lc_lds; csrc/tps_plan.h decides, csrc/tps_device.h carve_fused /
tile_lc_s / binseg_from_lc) in the host emulation: every batch of tests/lc_lds_cases.py scanned with PlanKnobs::lc_lds on and off
(tests/emu_lc_lds_driver.py).  The resident path must have run exactly where the plan says so (emulation counter 15), both scans
must agree bit for bit in results (bkp, gain, flags, n_win, ...) and in every S_w, and both must equal the C oracle
(kernel_matrix.check_scan)."""
import numpy as np
import pytest

import emu_lc_lds_driver as eld
import kernel_matrix as km
import lc_lds_cases as lc
import test_kernel_matrix as tkm
from topsicle_amd import hiplib


def _max_nwin(case):
    row = case.row
    return max(hiplib.window_count(len(x), row.W, row.s, row.t, row.M) for x in case.reads)


def test_the_cases_are_what_they_claim():
    by_id = {c.id: c for c in lc.CASES}
    row = by_id["tile_edges"].row
    assert row.tw == 494 and lc.length(3301, row) == 20000 == row.M
    assert sorted(hiplib.window_count(len(x), row.W, row.s, row.t, row.M) for x in by_id["tile_edges"].reads) == sorted(lc.TILE_EDGES + (37,))
    P = len(row.patterns)
    assert P == 12 and 65 * 9 * (96 + P) < 65536 <= 65 * 10 * (96 + P)
    assert _max_nwin(by_id["capacity_exact"]) // 4 + 4 == lc.ENTRIES == _max_nwin(by_id["capacity_one_over"]) // 4 + 3
    s, _ = km.occ.window_counts(by_id["wrap_around"].reads[0], "forward", row.patterns, row.W, row.s, row.t, row.M)
    assert len(s) == 3301 and int(np.sum(s)) > 4 * 65536
    s, _ = km.occ.window_counts("A" * 2500, "reverse", row.patterns, row.W, row.s, row.t, row.M)
    assert set(np.asarray(s).tolist()) == {P}


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_plan(case):
    pl = eld.planned(case.row.patterns, case.row.params(), _max_nwin(case), val_on=case.dirty)
    assert pl["entries"] == lc.ENTRIES
    assert bool(pl["lc_lds"]) == case.resident, pl
    if case.id.startswith("capacity"):
        assert pl["lc_cap"] + 2 == lc.ENTRIES + (0 if case.resident else 1), pl


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_resident_equals_off_chip_equals_oracle(case):
    row, reads = case.row, case.reads
    with eld.scanning(True) as on:
        a = tkm.emu_scan(row, reads, dirty=case.dirty)
    with eld.scanning(False) as off:
        b = tkm.emu_scan(row, reads, dirty=case.dirty)
    assert off[eld.LDS_CANDS] == 0 and off[eld.LANE_CANDS] == on[eld.LANE_CANDS], (on, off)
    if case.resident:
        assert on[eld.LDS_CANDS] == on[eld.LANE_CANDS] > 0, on          # every tile that stored its lanes' candidates kept them in LDS
    else:
        assert on[eld.LDS_CANDS] == 0, on
    idx = np.arange(len(reads))
    km.same_outputs(a, b, idx, idx, case.id + ": resident against off-chip")
    assert a["results"]["gain"].tobytes() == b["results"]["gain"].tobytes()
    km.check_scan(a, row, reads, "resident")
    km.check_scan(b, row, reads, "off-chip")
    tied = (a["results"]["flags"] & hiplib.RES_TIE) != 0
    for i in case.ties:
        assert tied[i], (case.id, i, "the exact tournament decides this read")
    if case.ties:
        assert on[eld.EXACT_TOURNAMENTS] >= len(case.ties) and on[eld.EXACT_TOURNAMENTS] == off[eld.EXACT_TOURNAMENTS], (on, off)
