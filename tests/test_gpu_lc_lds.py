"""Resident candidate sums of the default kernels (ScanArgs::lc_lds) on the device: every batch of tests/lc_lds_cases.py scanned
twice by tps_scan_kernel_s6p, as the library plans it and with the debug option lc_lds = 0 (the off-chip layout in the same
library).  Results and window sums must be byte-identical, and both equal to the C oracle (kernel_matrix.check_scan; the reads the
exact tournament decides carry TPS_RES_TIE in both -- with resident sums the fence in front of the wave's own S_w stands on that
path only).  kernel_info does not show the mode: which one the library planned is taken from the emulation library's planner call,
the same plan_geometry with the knobs of the library's contexts (tests/emu_lc_lds_driver.py)."""
import numpy as np
import pytest

import emu_lc_lds_driver as eld
import kernel_matrix as km
import lc_lds_cases as lc
from topsicle_amd import hiplib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    s = hiplib.HipScanner(0)
    yield s
    s.close()


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_resident_equals_off_chip_equals_oracle(sc, case):
    from test_gpu_kernel_matrix import gpu_scan
    row, reads = case.row, case.reads
    assert len(reads) <= 64
    max_nwin = max(hiplib.window_count(len(x), row.W, row.s, row.t, row.M) for x in reads)
    assert bool(eld.planned(row.patterns, row.params(), max_nwin, val_on=case.dirty)["lc_lds"]) == case.resident
    outs = []
    try:
        for mode in (1, 0):
            sc.debug_option("lc_lds", mode)
            out, info = gpu_scan(sc, 0, row, reads, twice=True)
            assert info.split(" lds=")[0] == lc.KERNEL, info
            outs.append((out, info))
    finally:
        sc.debug_option("lc_lds", 1)
    (a, info_a), (b, info_b) = outs
    assert info_a == info_b, "the resident layout costs no LDS byte and no workgroup"
    idx = np.arange(len(reads))
    km.same_outputs(a, b, idx, idx, case.id + ": resident against off-chip")
    assert a["results"]["gain"].tobytes() == b["results"]["gain"].tobytes()
    km.check_scan(a, row, reads, "resident")
    km.check_scan(b, row, reads, "off-chip")
    tied = (a["results"]["flags"] & hiplib.RES_TIE) != 0
    for i in case.ties:
        assert tied[i], (case.id, i, "the exact tournament decides this read")
