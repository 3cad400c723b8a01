"""Step 1 of the pair-table kernels (trc_decide_pairs) on the MI355X: the cases of step1_pairs_cases.py, scanned with F_STEP1
alone, against the C oracle bit for bit; the launched kernel is asserted to be the pair-table kernel of the case's slide.
test_step1_pairs.py runs the same cases through the host emulation and asserts the route every read takes."""
import numpy as np
import pytest

import step1_pairs_cases as sp
from topsicle_amd import hiplib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    s = hiplib.HipScanner(0)
    yield s
    s.close()


@pytest.mark.parametrize("case", sp.CASES, ids=lambda c: c.id)
def test_case(sc, case):
    if sc.patterns != case.patterns:
        sc.set_patterns(case.patterns)
    bases, offsets = hiplib.pack_reads(case.reads)
    sc.upload(0, bases, offsets)
    outs = []
    for _ in range(2):                       # (the second scan reuses the cached plan)
        sc.scan(0, case.params())
        sc.sync()
        res = sc.results(0).copy()
        cs, ce = sc.batch_trc_counts(0)
        outs.append((res, cs, ce))
    info = sc.kernel_info(0)
    assert info.split(" lds=")[0] == "tps_scan_kernel_s%d%s" % (case.slide, case.kernel_suffix), info
    n_pass = sp.check(case, *outs[0], "gpu")
    assert 0 < n_pass < len(case.reads)
    assert outs[0][0].tobytes() == outs[1][0].tobytes()
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
