"""The scan-kernel matrix (tests/kernel_matrix.py) on the MI355X: every row is scanned on a clean batch and on a dirty one,
the launched kernel is asserted by its exact name, and every output is compared with the C oracle (step-1 counts, the
decision, window offsets, every S_w, every raw row, the change point).  A second scan of the same slot (the cached plan)
must give the same bytes, and so must the clean reads inside the dirty batch (the fallback tile against the fast one).
The knob tests hold the outputs byte-identical across workgroup shapes, the self-overlap tiles' order, a kept pair table
and the dispatch order."""
import time

import numpy as np
import pytest

import kernel_matrix as km
from topsicle_amd import hiplib

pytestmark = pytest.mark.gpu
_seen = {"names": set(), "rows": 0, "reads": 0, "windows": 0, "t0": None}


@pytest.fixture(scope="module")
def sc():
    s = hiplib.HipScanner(0)
    yield s
    s.close()


def _set_knobs(sc, knobs):
    for key in ("force_generic", "force_pair", "so_order", "wpg", "file_order"):
        sc.debug_option(key, int(knobs.get(key, 0)))


def gpu_scan(sc, slot, row, reads, knobs=None, twice=False):
    """Upload, scan (twice: the second reuses the cached plan) and download; returns (outputs, kernel_info)."""
    _set_knobs(sc, dict(row.knobs, **(knobs or {})))
    if sc.patterns != row.patterns:
        sc.set_patterns(row.patterns)
    bases, offsets = hiplib.pack_reads(reads)
    sc.upload(slot, bases, offsets)
    outs = []
    for _ in range(2 if twice else 1):
        sc.scan(slot, row.params())
        sc.sync()
        res = sc.results(slot).copy()
        sums, win_off = sc.window_sums(slot)
        cs, ce = sc.batch_trc_counts(slot)
        out = dict(results=res, sums=sums, win_off=win_off, c_start=cs, c_end=ce,
                   raw=sc.window_raw(slot)[0] if row.raw else None)
        resolved = res.copy()
        hiplib.resolve_ties(sc, slot, resolved, len(row.patterns), row.jump, row.min_size)
        out["bkp_resolved"] = resolved["bkp"]
        outs.append(out)
    info = sc.kernel_info(slot)
    _set_knobs(sc, {})
    if twice:
        km.same_outputs(outs[0], outs[1], np.arange(len(reads)), np.arange(len(reads)), row.id + " second scan")
    return outs[0], info


def _batches(row):
    clean, dirty, _ = km.edge_reads(row)
    lo = len(dirty) // 2
    return clean, dirty[:lo] + clean + dirty[lo:], lo


@pytest.mark.parametrize("row", km.ROWS, ids=lambda r: r.id)
def test_row(sc, row):
    if _seen["t0"] is None:
        _seen["t0"] = time.time()
    clean, batch, lo = _batches(row)
    a, info = gpu_scan(sc, 0, row, clean, twice=True)
    assert info.split(" lds=")[0] == row.expected(False), info
    n, w = km.check_scan(a, row, clean, "clean")
    b, info = gpu_scan(sc, 1, row, batch, twice=True)
    assert info.split(" lds=")[0] == row.expected(True), info
    n2, w2 = km.check_scan(b, row, batch, "dirty")
    km.same_outputs(a, b, np.arange(len(clean)), np.arange(lo, lo + len(clean)), row.id + " clean reads in a dirty batch")
    _seen["names"] |= {row.expected(False), row.expected(True)}
    _seen["rows"] += 1
    _seen["reads"] += n + n2
    _seen["windows"] += w + w2


def test_all_kernels_asserted():
    """Runs after the rows: with every row run, every declared kernel was asserted by name on the device."""
    if _seen["rows"] != len(km.ROWS):
        pytest.skip("only part of the matrix ran")
    import test_kernel_matrix as tkm
    assert _seen["names"] == set(tkm.declared_kernels())
    print(f"\nkernel matrix: {_seen['rows']} rows, {len(_seen['names'])} kernels asserted, {_seen['reads']} reads and "
          f"{_seen['windows']} windows compared with the oracle, {time.time() - _seen['t0']:.1f} s")
    print(" ".join(sorted(_seen["names"])))


def _identical(sc, row, knobs_a, knobs_b):
    for dirty in (False, True):
        clean, batch, _ = _batches(row)
        reads = batch if dirty else clean
        a, ia = gpu_scan(sc, 2, row, reads, knobs_a)
        b, ib = gpu_scan(sc, 3, row, reads, knobs_b)
        idx = np.arange(len(reads))
        km.same_outputs(a, b, idx, idx, f"{row.id} {knobs_a} vs {knobs_b} dirty={dirty}")
        assert np.array_equal(a["win_off"], b["win_off"])
        yield dirty, ia, ib


FAMILY_ROWS = ["plain_s6", "p_s6", "r_s6", "so_s6", "sol_s6", "sor_s6", "sorh_s6", "q_s6", "sixteen_s6", "p_s10", "so_s6_W262"]


@pytest.mark.parametrize("rid", FAMILY_ROWS)
def test_workgroup_shapes_identical(sc, rid):
    """Both shapes must really run on every fused kernel (8 waves of these tables fit the LDS: the planner accepts the knob);
    the generic kernel (the sixteen-pattern table on a dirty batch) ignores it."""
    row = km.BY_ID[rid]
    for dirty, ia, ib in _identical(sc, row, {"wpg": 4}, {"wpg": 8}):
        if row.expected(dirty) != km.GENERIC:
            assert ia.endswith(" waves_per_wg=4") and ib.endswith(" waves_per_wg=8"), (dirty, ia, ib)


@pytest.mark.parametrize("rid", ["sor_s5", "sor_s6", "sor_s7", "sor_s8", "sorh_s5", "sorh_s6", "sorh_s7", "sorh_s8", "sor_s6_W157", "sorh_s6_W93"])
def test_self_overlap_tile_order_identical(sc, rid):
    for _ in _identical(sc, km.BY_ID[rid], {}, {"so_order": 2}):
        pass


@pytest.mark.parametrize("rid", ["q_s5", "q_s6", "q_s8", "p_s6", "p_s12", "r_s6", "p_s6_W157"])
def test_kept_pair_table_identical(sc, rid):
    for _ in _identical(sc, km.BY_ID[rid], {}, {"force_pair": 1}):
        pass


@pytest.mark.parametrize("rid", ["p_s6", "so_s6", "sorh_s6", "q_s7", "p_s6_M4000"])
def test_dispatch_order_identical(sc, rid):
    """The edge reads are ragged (0 .. 2 maxlen bases): the planner reorders them unless file_order is set."""
    for _ in _identical(sc, km.BY_ID[rid], {}, {"file_order": 1}):
        pass
