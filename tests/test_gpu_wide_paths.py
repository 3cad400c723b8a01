"""The wide-table kernel's path matrix (tests/wide_path_rows.py) on the MI355X, everything through hiplib.HipScanner: every
row is scanned twice (the second scan reuses the cached plan), must launch tps_scan_kernel_wide with exactly the LDS the
emulation's planner gives for the device's budget, and every output is compared with oracle/oracle.c (step-1 counts, the
decision, window offsets, every S_w, every raw byte, the change point).  The capacity boundary is derived for the device's own
budget: the largest head the plan accepts scans (with more than 64 KB of LDS per workgroup), 64 bases more is refused.  On top:
the dispatch order changes no byte, and the one-shot step-1 call plans the same large tile."""
import re

import numpy as np
import pytest

import emu_wide_driver as emuw
import wide_path_rows as wp
from topsicle_amd import hiplib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    s = hiplib.HipScanner(0)
    yield s
    s.close()


def lds_budget(sc):
    """What do_scan plans the wide kernel with: min(LDS per block of the device, 160 KB)."""
    return min(int(re.search(r"LDS/block=(\d+)", sc.device_info()).group(1)), 160 * 1024)


def gpu_scan(sc, slot, row, reads, prm, tails=None, file_order=0, times=1):
    sc.debug_option("file_order", file_order)
    try:
        if sc.patterns != row.patterns:
            sc.set_patterns_wide(row.patterns)
        sc.upload(slot, *hiplib.pack_reads(reads))
        if tails is not None:
            sc.set_tails(slot, tails)
        outs = []
        for _ in range(times):
            sc.scan(slot, prm)
            sc.sync()
            res = sc.results(slot).copy()
            out = dict(results=res, win_off=sc.window_offsets(slot))
            if prm.flags & hiplib.F_STEP1:
                out["c_start"], out["c_end"] = sc.batch_trc_counts(slot)
            if prm.flags & hiplib.F_WINDOWS:
                out["sums"], _ = sc.window_sums(slot)
                resolved = res.copy()
                hiplib.resolve_ties(sc, slot, resolved, len(row.patterns), row.jump, row.min_size)
                out["bkp_resolved"] = resolved["bkp"]
            if prm.flags & hiplib.F_STORE_RAW:
                out["raw"], _ = sc.window_raw(slot)
            outs.append(out)
        info = sc.kernel_info(slot)
    finally:
        sc.debug_option("file_order", 0)
    for o in outs[1:]:
        same_outputs(outs[0], o, row.id + " second scan")
    return outs[0], info


def same_outputs(a, b, tag):
    """Byte identity of two scans of one batch.  (The mask is from before the downloads handed out zeros for reads that do not
    pass; tests/test_gpu_poison.py compares these rows unmasked.)"""
    assert a["results"].tobytes() == b["results"].tobytes(), (tag, "results")
    assert np.array_equal(a["win_off"], b["win_off"]), tag
    for key in ("c_start", "c_end"):
        if key in a:
            assert a[key].tobytes() == b[key].tobytes(), (tag, key)
    keep = np.repeat(a["results"]["pass"].astype(bool), np.diff(a["win_off"]))
    for key in ("sums", "raw"):
        if key in a:
            assert a[key][keep].tobytes() == b[key][keep].tobytes(), (tag, key)


def run_row(sc, row, slot=0):
    """Scan `row` and compare with the oracle; returns (windows compared, lds bytes), or (0, 0) after a refusal row's refusal."""
    reads = wp.reads_of(row)
    prm = wp.params_of(row, reads)
    tails = wp.tails_of(row, reads) if prm.flags & hiplib.F_TAILS_IN else None
    if row.refuse:
        with pytest.raises(hiplib.TopsicleHipError) as e:
            gpu_scan(sc, slot, row, reads, prm, tails)
        assert wp.error_code(e.value) == row.refuse, str(e.value)
        return 0, 0
    out, info = gpu_scan(sc, slot, row, reads, prm, tails, times=2)
    pl = emuw.plan(row.patterns, prm, lds_budget(sc))
    assert (pl["tp_cap"], pl["tw"]) == (row.tp_cap, row.tw), (row.id, pl)
    assert info.startswith(wp.WIDE + " lds=%d " % pl["lds_bytes"]) and info.endswith(" waves_per_wg=4"), (row.id, info, pl)
    windows = wp.check_scan(out, row, reads, prm, tails)
    if prm.flags & hiplib.F_WINDOWS:
        assert windows > 0, row.id
    else:
        assert out["c_start"].sum() + out["c_end"].sum() > 0 or row.no_bp < row.k, row.id
    return windows, pl["lds_bytes"]


@pytest.mark.parametrize("row", wp.ROWS, ids=lambda r: r.id)
def test_row(sc, row):
    windows, lds = run_row(sc, row, slot=len(row.id) % 3)
    if row.id.startswith("nobp8000") and row.flags & hiplib.F_STEP1:
        assert lds > 65536, (row.id, lds)              # the raised dynamic-LDS limit is really launched


@pytest.mark.parametrize("which", range(len(wp.BOUNDARY_TABLES)))
def test_capacity_boundary_of_this_device(sc, which):
    """The largest head the plan accepts at this device's budget scans like the oracle, with more than 64 KB of LDS per
    workgroup; 64 bases more is TPS_E_CAPACITY."""
    budget = lds_budget(sc)
    acc, ref, pl = wp.boundary_rows(budget, emuw.plan)[which]
    print(f"\n{acc.id}: budget {budget}, tp_cap {pl['tp_cap']}, tw {pl['tw']}, lds {pl['lds_bytes']}, n_so {pl['n_so']}")
    windows, lds = run_row(sc, acc, slot=3)
    assert windows > 0 and 65536 < lds == pl["lds_bytes"] <= budget
    run_row(sc, ref, slot=3)


@pytest.mark.parametrize("rid", ["nobp8000", "nobp8000_acac_sums", "W4098_s23"])
def test_dispatch_order_changes_no_byte(sc, rid):
    """A raw row and a sums row of 8000-base tiles, and a row of 3-window tiles: the edge reads are ragged (0 .. 1.5 maxlen bases), so
    the planner reorders them unless file_order is set (WideArgs::order)."""
    row = wp.BY_ID[rid]
    reads = wp.reads_of(row)
    prm = wp.params_of(row, reads)
    nw = {hiplib.window_count(len(x), row.W, row.s, row.t, row.M) for x in reads}
    assert len(nw) > 4
    a, _ = gpu_scan(sc, 4, row, reads, prm, file_order=0)
    b, _ = gpu_scan(sc, 5, row, reads, prm, file_order=1)
    same_outputs(a, b, rid + " file_order 0 against 1")
    assert wp.check_scan(b, row, reads, prm) > 0


@pytest.mark.parametrize("tab", ["m23k21", "acac16"])
def test_one_shot_step1_with_a_4097_base_head(sc, tab):
    """tps_trc_counts on a wide table plans its own scan (tp_cap = 4160): the counts are the batch's and the oracle's."""
    row = wp.BY_ID[f"{tab}_head4097_step1"]
    reads = wp.reads_of(row) + wp.reads_of(wp.BY_ID["dirty_m23" if tab == "m23k21" else "dirty_acac_s23"])[:6]
    out, info = gpu_scan(sc, 0, row, reads, row.params())
    cs, ce = sc.trc_counts(*hiplib.pack_reads(reads), no_bp=4097)
    assert np.array_equal(cs, out["c_start"]) and np.array_equal(ce, out["c_end"])
    for i, seq in enumerate(reads):
        want = wp.step1_of(row, seq)
        assert (cs[i].tolist(), ce[i].tolist()) == want, (tab, i)
    assert cs.max() > 150 and ce.max() > 150
