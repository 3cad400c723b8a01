"""Step 1 of the pair-table kernels (trc_decide_pairs) through the host emulation: the cases of step1_pairs_cases.py against
the C oracle bit for bit, and for every read the route the kernel took -- so that no case silently tests the old count.
The emulation's planner can drop a pair table the device keeps, so the cases plan with the knob force_pair, as
test_kernel_matrix.py does for the `_s*p` / `_s*q` rows."""
import numpy as np
import pytest

import emu_binseg_driver as ebd
import emu_driver as emu
import step1_pairs_cases as sp


def _scan(case, reads):
    emu.KNOBS.update(val_off=0 if sp.is_dirty(case) else 1, force_pair=1)
    try:
        return emu.scan(case.patterns, reads, case.params())
    finally:
        emu.KNOBS.update(val_off=0, force_pair=0)


def _plan(case):
    emu.KNOBS.update(val_off=0 if sp.is_dirty(case) else 1, force_pair=1)
    try:
        return emu.plan_table(case.patterns, case.params(), 4000)
    finally:
        emu.KNOBS.update(val_off=0, force_pair=0)


@pytest.mark.parametrize("case", sp.CASES, ids=lambda c: c.id)
def test_shapes(case):
    sp.check_shapes(case)


@pytest.mark.parametrize("case", sp.CASES, ids=lambda c: c.id)
def test_emulation(case):
    pl = _plan(case)
    assert pl["variant"] == case.slide and pl["pair_n"] > 0, pl
    with ebd.counting() as got:
        out = _scan(case, case.reads)
    n_pass = sp.check(case, out["results"], out["c_start"], out["c_end"], "emulation")
    assert 0 < n_pass < len(case.reads)
    want = [sp.expected_route(case, x) for x in case.reads]
    assert got[sp.PAIRS] == sum(w == sp.PAIRS for w in want), (got, case.id)
    assert got[sp.PAIRS] + got[sp.PACKED] + got[sp.HIST] == len(case.reads)
    # ... and read by read: each one alone takes the route expected of it, and gives the bytes it gave in the batch
    for i, seq in enumerate(case.reads):
        with ebd.counting() as one:
            o = _scan(case, [seq])
        routes = {c: one[c] for c in (sp.PAIRS, sp.PACKED, sp.HIST)}
        assert sum(routes.values()) == 1, (case.id, i, routes)
        assert (routes[sp.PAIRS] == 1) == (want[i] == sp.PAIRS), (case.id, i, len(seq), routes)
        assert o["results"].tobytes() == out["results"][i:i + 1].tobytes(), (case.id, i)
        assert np.array_equal(o["c_start"][0], out["c_start"][i]) and np.array_equal(o["c_end"][0], out["c_end"][i]), (case.id, i)


def test_both_routes_are_exercised():
    """Across the cases: most reads take the new route, and the bound, k = 3 with long heads and dirty heads keep the old ones."""
    want = {c.id: [sp.expected_route(c, x) for x in c.reads] for c in sp.CASES}
    assert all(w == sp.PAIRS for w in want["k4_P12_nobp1023"])
    assert any(w == sp.PAIRS for w in want["k4_P12_nobp1024"]) and any(w is None for w in want["k4_P12_nobp1024"])
    assert any(w == sp.PAIRS for w in want["k3_P10_nobp1000"]) and any(w is None for w in want["k3_P10_nobp1000"])
    assert all(w == sp.PAIRS for w in want["k3_P10_nobp700"])
    assert all(w is None for w in want["k2_P3_nobp400"])
    for cid in ("k4_P12_s6_dirty", "k5_P14_s6_dirty"):
        assert 0 < sum(w is None for w in want[cid]) < len(want[cid]) // 4
