"""The scan-kernel matrix (tests/kernel_matrix.py) on the host: every kernel the library declares has rows, the planner
picks for every row the plan its expected kernel needs, and every row's scan through the host emulation of the kernel
source equals the C oracle -- on a clean batch, on a dirty one, and with the clean reads identical in both.  The GPU half
(test_gpu_kernel_matrix.py) runs the same rows on the MI355X and asserts the kernels by name.

The emulation differs from the device build where tps_plan.h / tps_device.h say `#ifndef TPS_EMU`.  For the planner
that is `seq_alias` (the default kernels keep the staged bases in the tail of row[] on the device): the emulation's wave
slices are larger, so the pair-table rule, which weighs resident workgroups, can drop a pair table the device keeps.
Rows whose device kernel has a pair table (`_s*p`, `_s*q`) therefore plan and run here with the planner knob
force_pair, which keeps it."""
import os
import re

import numpy as np
import pytest

import emu_driver as emu
import kernel_matrix as km
from topsicle_amd import hiplib

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "topsicle_amd", "csrc")


def declared_kernels():
    src = open(os.path.join(CSRC, "tps_kernels.h")).read()
    return re.findall(r"^TPS_SCAN_KERNEL_DECL\((\w+)\)", src, re.M)


def launched_names():
    """The kernels the host's table names (topsicle_hip.hip: TPS_K(symbol) gives the function and, stringized, the reported name)."""
    src = open(os.path.join(CSRC, "topsicle_hip.hip")).read()
    return re.findall(r"\bTPS_K\((tps_\w+)\)", src)


def test_every_kernel_has_a_clean_and_a_dirty_row():
    decl = declared_kernels()
    assert len(decl) == len(set(decl)) == 45, decl          # the generic kernel, 8 families x slides 5 .. 8, 2 x 6 other slides
    names = launched_names()
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)       # each symbol is written once
    assert set(names) == set(decl)
    clean = {r.expected(False) for r in km.ROWS}
    dirty = {r.expected(True) for r in km.ROWS}
    assert set(decl) - clean == set(), sorted(set(decl) - clean)
    assert set(decl) - dirty == set(), sorted(set(decl) - dirty)
    assert clean | dirty <= set(decl)
    ids = [r.id for r in km.ROWS]
    assert len(ids) == len(set(ids))


def _pair_kernel(name):
    return name != km.GENERIC and (name.endswith("p") or name.endswith("q"))


def _plan(row, dirty):
    emu.KNOBS.update(val_off=0 if dirty else 1, force_pair=1 if _pair_kernel(row.expected(dirty)) else 0)
    try:
        nw = hiplib.window_count(2 * row.M, row.W, row.s, row.t, row.M)
        pl = emu.plan_table(row.patterns, row.params(), nw)
        stride = emu.stride_base(row.patterns, row.params(), 2 * row.M)
    finally:
        emu.KNOBS.update(val_off=0, force_pair=0)
    return pl, stride


def kernel_of_plan(row, pl):
    """The kernel do_scan (topsicle_hip.hip) launches for a plan: the family by table and outputs, then the slide."""
    if row.knobs.get("force_generic") or pl["variant"] == 0:
        return km.GENERIC
    v, pair = pl["variant"], pl["pair_n"] > 0
    so = any(km.periods(p) for p in row.patterns)
    if v not in (5, 6, 7, 8):
        return "tps_scan_kernel_s%d%s" % (v, "p" if pair else "")
    if so:
        fam = ("sorh" if row.k >= 6 and pl["pp_d"] > 0 else "sor") if row.raw else ("sol" if 2 <= pl["pp_d"] <= 4 else "so")
    else:
        fam = "r" if row.raw else ("q" if pair and row.k == 5 else "p" if pair else "plain")
    return km.kname(fam, v)


@pytest.mark.parametrize("row", km.ROWS, ids=lambda r: r.id)
def test_plan(row):
    for dirty in (False, True):
        pl, stride = _plan(row, dirty)
        assert kernel_of_plan(row, pl) == row.expected(dirty), (dirty, pl)
        assert stride == 0, "a strided scan would name its base kernel"
        if pl["variant"]:
            assert pl["tw"] == row.tw, pl
        name = row.expected(dirty)
        if name.endswith(("sol", "sor")):
            assert pl["pp_d"] == 4
        if name.endswith(("so", "sorh")):
            assert pl["pp_d"] == 5
        if row.family == "r" and row.s == 6:
            assert (pl["pair_n"] > 0) == ((row.W - row.k) % 6 == 0), "the raw rows' pair table of fields needs r = 0"


def test_planner_boundaries():
    """NOBP_MAX / W_MAX are the largest no_bp / window that still plan a fused kernel at slide 6 for the k = 4 table."""
    def fused(**kw):
        row = km.Row("x", "p", **kw)
        return _plan(row, False)[0]["variant"] != 0
    assert fused(no_bp=km.NOBP_MAX) and not fused(no_bp=km.NOBP_MAX + 1)
    assert fused(W=km.W_MAX) and not fused(W=km.W_MAX + 1)


@pytest.mark.parametrize("row", [r for r in km.ROWS if r.jump == 5 and r.min_size == 2 and not r.knobs and not r.filt], ids=lambda r: r.id)
def test_edge_reads_shapes(row):
    """The reads are on the edges they claim: window counts on the tile boundaries, and every dirty letter at its offset in
    the coordinates of the tail step 1 picks for the dirty read (a window holds W - 1 characters of the scanned string)."""
    clean, dirty, marks = km.edge_reads(row)
    assert 40 <= len(clean) + len(dirty) <= 80
    assert all(set(x) <= set("ACGT") for x in clean)
    assert all(set(x) - set("ACGT") for x in dirty) and len(marks) == len(dirty)
    nw = {hiplib.window_count(len(x), row.W, row.s, row.t, row.M) for x in clean}
    full = {0, 1, 2, 6, 7, 8, 9, 16, 17}
    if row.M >= row.t + row.W + 2 * row.tw * row.s:
        full |= {row.tw - 1, row.tw, row.tw + 1, 2 * row.tw, 2 * row.tw + 1}
    assert full <= nw
    kinds = set()
    for seq, m in zip(dirty, marks):
        if m.tail is None:
            continue
        L = len(seq)
        bad = [i for i, c in enumerate(seq) if c not in "ACGT"]
        assert bad == [m.pos], (m, bad)
        assert km.tail_of(seq, row) == m.tail, m
        kinds.add((m.kind, m.tail))
        x = m.pos - row.t if m.tail == 0 else L - 1 - row.t - m.pos
        if m.x is not None:
            assert x == m.x
            nwin = hiplib.window_count(L, row.W, row.s, row.t, row.M)
            assert 0 <= x <= (nwin - 1) * row.s + row.W - 2
        if m.kind.startswith("window 3's"):
            assert x == 3 * row.s + (row.W - 2 if "last" in m.kind else 0)
        if m.kind.startswith("tile 1's"):
            assert x == row.tw * row.s + (row.W - 2 if "last" in m.kind else 0)
        if m.kind.startswith("tile 2's"):
            assert x == 2 * row.tw * row.s
        want = {"first base": 0, "last base": L - 1, "start head's last base": row.no_bp - 1,
                "end head's first base": L - row.no_bp, "base before the end head": L - row.no_bp - 1}.get(m.kind)
        if want is not None:
            assert m.pos == want, m
    for tail in (0, 1):
        assert {("window 0's first base", tail), ("window 3's last base", tail), ("end head's first base", tail)} <= kinds
        if row.M >= row.t + row.W + 2 * row.tw * row.s:
            assert {("tile 1's first window's first base", tail), ("tile 1's first window's last base", tail),
                    ("tile 2's first window's first base", tail)} <= kinds


def emu_scan(row, reads, dirty, knobs=None):
    knobs = dict(row.knobs, **(knobs or {}))
    emu.KNOBS.update(val_off=0 if dirty else 1, force_pair=1 if _pair_kernel(row.expected(dirty)) else knobs.get("force_pair", 0),
                     so_order=knobs.get("so_order", 0))
    try:
        out = emu.scan(row.patterns, reads, row.params(), force_generic=knobs.get("force_generic", 0))
    finally:
        emu.KNOBS.update(val_off=0, force_pair=0, so_order=0)
    tot = int(out["win_off"][-1])
    out["raw"] = out["raw"] if row.raw else None
    out["bkp_resolved"] = km.resolve_with(out["sums"], out["win_off"], out["results"], len(row.patterns), row.jump, row.min_size)
    assert len(out["sums"]) == tot
    return out


def reduced(reads):
    """The emulation's read set: every edge shape but the longest reads (2 maxlen) -- the GPU half runs them all."""
    return [x for x in reads if len(x) <= 25000]


@pytest.mark.parametrize("row", km.ROWS, ids=lambda r: r.id)
def test_emulation(row):
    clean, dirty, _ = km.edge_reads(row)
    clean = reduced(clean)
    a = emu_scan(row, clean, dirty=False)
    km.check_scan(a, row, clean, "clean")
    batch = dirty[: len(dirty) // 2] + clean + dirty[len(dirty) // 2:]
    b = emu_scan(row, batch, dirty=True)
    km.check_scan(b, row, batch, "dirty")
    lo = len(dirty) // 2
    km.same_outputs(a, b, np.arange(len(clean)), np.arange(lo, lo + len(clean)), row.id + " clean reads in a dirty batch")
