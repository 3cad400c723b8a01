"""The wide-table kernel's path matrix (tests/wide_path_rows.py) on the host: plan_wide gives every row the plan its literals
name, the rows reach the shapes they promise, and every row's scan through the host emulation of csrc/tps_wide.h equals
oracle/oracle.c field by field.  The GPU half (test_gpu_wide_paths.py) runs the same rows on the MI355X."""
import subprocess

import numpy as np
import pytest

import emu_wide_driver as emuw
import wide_path_rows as wp
from topsicle_amd import hiplib

BUDGET = emuw.LDS_BUDGET          # the emulation's scan plans with the MI355X's 160 KB per workgroup


def emu_scan(row, reads, prm, tails=None, base_shift=0):
    out = emuw.scan(row.patterns, reads, prm, tails=tails, base_shift=base_shift)
    out["bkp_resolved"] = wp.resolve_with(out["sums"], out["win_off"], out["results"], len(row.patterns), row.jump, row.min_size)
    return out


def run_row(row, base_shift=0):
    reads = wp.reads_of(row)
    prm = wp.params_of(row, reads)
    tails = wp.tails_of(row, reads) if prm.flags & hiplib.F_TAILS_IN else None
    if row.refuse:
        with pytest.raises(hiplib.TopsicleHipError) as e:
            emu_scan(row, reads, prm, tails)
        assert wp.error_code(e.value) == row.refuse, str(e.value)
        return 0
    out = emu_scan(row, reads, prm, tails, base_shift)
    windows = wp.check_scan(out, row, reads, prm, tails)
    if prm.flags & hiplib.F_WINDOWS:
        assert windows > 0, row.id
    else:
        assert out["c_start"].sum() + out["c_end"].sum() > 0 or row.no_bp < row.k, row.id
    return windows


def test_planner_gives_every_row_its_plan():
    """Every row's tp_cap and tw are literals; plan_wide must agree.  The rows and the boundary rows together show four causes of
    tp_cap (the floor, the window, the head, the largest accepted) and the three kinds of tw."""
    print()
    tps, tws = set(), set()
    for row in wp.ROWS:
        pl = emuw.plan(row.patterns, row.params(), BUDGET)
        if row.refuse:
            assert pl.get("error") == row.refuse, (row.id, pl)
            print(f"{row.id:32s} refused: {pl['message']}")
            continue
        assert "error" not in pl, (row.id, pl)
        print(f"{row.id:32s} tp_cap={pl['tp_cap']:6d} tw={pl['tw']:5d} seq_dw={pl['seq_dw']:5d} lds={pl['lds_bytes']:6d}")
        assert (pl["tp_cap"], pl["tw"]) == (row.tp_cap, row.tw), (row.id, pl)
        assert pl["wpg"] == 4
        tps.add(pl["tp_cap"])
        tws.add(pl["tw"])
    by_window = {r.tp_cap for r in wp.SCAN_ROWS if r.W - 1 > 4096 and r.W - 1 > r.no_bp}
    by_head = {r.tp_cap for r in wp.SCAN_ROWS if r.flags & hiplib.F_STEP1 and r.no_bp > 4096 and r.no_bp > r.W - 1}
    assert 4096 in tps and by_window and by_head and min(by_window | by_head) > 4096
    assert 1 in tws and any(2 <= x < 64 for x in tws) and any(x >= 64 and x % 64 == 0 for x in tws)
    assert not any(x > 64 and x % 64 for x in tws)
    for acc, ref, pl in wp.boundary_rows(BUDGET, emuw.plan):
        print(f"{acc.id:32s} tp_cap={pl['tp_cap']:6d} tw={pl['tw']:5d} seq_dw={pl['seq_dw']:5d} lds={pl['lds_bytes']:6d} n_so={pl['n_so']}")
        assert pl["tp_cap"] == acc.no_bp > max(by_window | by_head) and pl["lds_bytes"] <= BUDGET
        tps.add(pl["tp_cap"])
    assert len(tps) >= 4


def test_capacity_boundary_depends_on_the_table():
    """The largest head the 160 KB plan accepts: far below WIDE_TP_MAX = 32768, and lower the more self-overlapping groups the
    table has (wide_nx_dw grows with n_so).  include/topsicle_hip.h and DESIGN.md quote these figures."""
    got = wp.boundary_rows(BUDGET, emuw.plan)
    assert [pl["n_so"] for _, _, pl in got] == [0, 4, 14]
    assert [acc.no_bp for acc, _, _ in got] == [25280, 24896, 24000]
    assert all(65536 < pl["lds_bytes"] <= BUDGET for _, _, pl in got)
    # a smaller budget moves the boundary: the rows are derived, not literals
    small = wp.boundary_rows(64 * 1024, emuw.plan)
    assert [acc.no_bp for acc, _, _ in small] == [7424, 7040, 6080] and all(pl["lds_bytes"] <= 65536 for _, _, pl in small)
    # the byte counters' limit through the plan alone: (W - 1) / k = 255 is the last one accepted
    for tab, W, ok in (("m23k21", 5376, True), ("m23k21", 5377, False), ("k1", 256, True), ("k1", 257, False), ("k2", 512, True), ("k2", 513, False)):
        pl = emuw.plan(wp.TABLES[tab][0], wp.Row("x", tab, W=W).params(), BUDGET)
        assert ("error" not in pl) == ok, (tab, W, pl)


def test_rows_reach_what_they_promise():
    ids = [r.id for r in wp.ROWS]
    assert len(ids) == len(set(ids))
    assert {r.table for r in wp.SCAN_ROWS} == set(wp.TABLES)
    assert {len(wp.TABLES[t][0]) for t in wp.TABLES} >= {2, 4, 12, 46, 64}
    for tab, n_so in (("m23k21", 14), ("m32k32", 20), ("acac16", 4), ("a20k18", 2), ("p64", 20), ("k1", 0), ("k2", 2), ("k3", 2)):
        assert emuw.table(wp.TABLES[tab][0])["n_so"] == n_so, tab
    assert {r.W - 1 for r in wp.SCAN_ROWS} >= {4095, 4096, 4097, 5000}
    assert {r.no_bp for r in wp.SCAN_ROWS} >= {1, 15, 16, 17, 20, 21, 22, 63, 64, 65, 999, 4096, 4097, 8000}
    assert {(r.jump, r.min_size) for r in wp.SCAN_ROWS} >= {(j, m) for j in (1, 3, 8, 13) for m in (1, 2, 4)}
    for r in wp.SCAN_ROWS:
        assert (r.W - 1) // r.k <= 255
    shapes = {("lw1=0" if r.W <= r.k else "lw1=1" if r.W == r.k + 1 else "s>lw1" if r.s > r.W - r.k else "s=lw1" if r.s == r.W - r.k else "s<lw1")
              for r in wp.SCAN_ROWS}
    assert shapes == {"lw1=0", "lw1=1", "s>lw1", "s=lw1", "s<lw1"}
    assert any((r.W - 1) // r.k == 255 and r.want_255 for r in wp.SCAN_ROWS if r.table == "k1")
    assert any((r.W - 1) // r.k == 255 and r.want_255 and r.unit == "A" for r in wp.SCAN_ROWS if r.table == "k2")
    assert {r.flags for r in wp.SCAN_ROWS} >= {wp.STEP1, wp.FULL, wp.RAW, wp.TAILS}


@pytest.mark.parametrize("row", [r for r in wp.SCAN_ROWS if r.reads == "edge"], ids=lambda r: r.id)
def test_edge_reads_shapes(row):
    """The window counts an edge row promises are there, each exactly and with bases left over; no read is longer than 30 kb."""
    reads = wp.reads_of(row)
    nw = {}
    for x in reads:
        n = hiplib.window_count(len(x), row.W, row.s, row.t, row.M)
        left = min(len(x), row.M) - row.t - row.W - (n - 1) * row.s if n else 0
        nw.setdefault(n, set()).add(left)
    tw = row.tw
    want = {0, 1, 2, 63, 64, 65, tw, tw + 1, 2 * tw, 2 * tw + 1} | ({tw - 1} if tw > 1 else set())
    assert want <= set(nw), sorted(want - set(nw))
    if row.s > 1:
        assert all(0 in nw[n] and len(nw[n]) > 1 for n in want if n), {n: nw[n] for n in want}
    lens = {len(x) for x in reads}
    assert {row.M - 1, row.M, row.M + 1, row.no_bp - 1, row.no_bp, row.no_bp + 1, 2 * row.no_bp - 1, 0, 1, row.k - 1, row.k} <= lens
    assert max(lens) <= 30000 and len(reads) <= 40


@pytest.mark.parametrize("row", [r for r in wp.SCAN_ROWS if r.reads == "dirty"], ids=lambda r: r.id)
def test_dirty_marks_are_where_they_claim(row):
    """Every dirty copy holds one non-ACGT letter, at its mark's offset in the coordinates of the tail step 1 picks for that copy."""
    reads, marks = wp.dirty_reads(row)
    assert len(reads) == len(marks) + 3 and set(reads[-1]) == {"N"}
    tw, s, W, t, nb = row.tw, row.s, row.W, row.t, row.no_bp
    assert nb == 4097
    kinds = set()
    for seq, m in zip(reads[2:], marks):
        L = len(seq)
        assert [i for i, c in enumerate(seq) if c not in "ACGT"] == [m.pos], m
        assert wp.decision(row, seq)[0] == m.tail, m
        nwin = hiplib.window_count(L, W, s, t, row.M)
        assert nwin > 2 * tw
        if m.x is not None:
            assert m.x == (m.pos - t if m.tail == 0 else L - 1 - t - m.pos) and 0 <= m.x <= (nwin - 1) * s + W - 2
        kinds.add((m.kind, m.tail))
    # tile 1 of a read with more than 2 tw windows is full: it stages tail characters [tw s, tw s + (tw - 1) s + W - 2]
    want = {"tile 1's first staged base": tw * s, "tile 1's last staged base": (2 * tw - 1) * s + W - 2,
            "tile 0's last window's last base": (tw - 1) * s + W - 2, "window 0's first base": 0}
    for m in marks:
        if m.kind in want:
            assert m.x == want[m.kind], m
    assert len(kinds) == 20 and {k for k, _ in kinds} >= set(want) | {"start head's first base", "start head's last base", "end head's first base", "end head's last base"}


@pytest.mark.parametrize("row", wp.ROWS, ids=lambda r: r.id)
def test_emulation(row):
    run_row(row, base_shift=len(row.id) % 4)


@pytest.mark.parametrize("which", range(len(wp.BOUNDARY_TABLES)))
def test_emulation_capacity_boundary(which):
    """The largest head the plan accepts scans like the oracle; 64 bases more is TPS_E_CAPACITY."""
    acc, ref, pl = wp.boundary_rows(BUDGET, emuw.plan)[which]
    assert run_row(acc) > 0
    run_row(ref)


def test_change_point_rows_hold_the_small_window_counts():
    seen = set()
    for row in (r for r in wp.SCAN_ROWS if r.reads == "binseg"):
        n = {hiplib.window_count(len(x), row.W, row.s, row.t, row.M) for x in wp.reads_of(row)}
        assert {1, 2, 3, 2 * row.min_size - 1, 2 * row.min_size, row.jump + 1} - {0} <= n, (row.id, sorted(n))
        seen |= n
    assert np.isin([1, 2, 3, 7, 8, 14], sorted(seen)).all()


def test_standalone_program_is_clean_under_sanitizers(tmp_path):
    """Every row, the boundary rows included, through the same kernel text under -fsanitize=address,undefined, as a program of
    its own: an LDS slice of exactly the planned size, output buffers of exactly the layout's size, the batch at all four
    alignments, and each scan's digest equal to that of the scan compared with the oracle above."""
    rows = list(wp.ROWS)
    for acc, ref, _ in wp.boundary_rows(BUDGET, emuw.plan):
        rows += [acc, ref]
    path = str(tmp_path / "rows.bin")
    wp.dump_rows(path, rows, emu_scan)
    out = subprocess.run([emuw.build_main(), path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip() == "ok: %d rows" % len(rows), out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
