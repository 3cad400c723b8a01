"""Windows aligned base by base on the GPU (tps_window_align; HipScanner.align_windows), through the C ABI: stat, cols and pile equal to
the plain restatement of the rule on the cases the emulation is checked on (tests/align_cases.py), bit for bit; with cols, the pile or
both not asked for; the same from launch to launch and under two fill bytes of the `poison` debug option; and every refusal with the
code and the words the emulation gives."""
import ctypes as C

import numpy as np
import pytest

import align_cases as ac
import emu_align_driver as emu
from topsicle_amd import hiplib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    with hiplib.HipScanner(0) as s:
        yield s


@pytest.mark.parametrize("name", ac.CASE_IDS)
def test_library_equals_oracle(sc, name):
    """(The first case is the first thing this context does: no tps_set_patterns has been called, no batch uploaded.)"""
    ac.assert_equal(ac.run_case(sc.align_windows, name), name)


@pytest.mark.parametrize("cols,pile", [(False, True), (True, False), (False, False)])
def test_pieces_not_asked_for(sc, cols, pile):
    for name in ("hand", "span17"):
        ac.assert_equal(ac.run_case(sc.align_windows, name, cols=cols, pile=pile), name, cols=cols, pile=pile)


def test_repeated_launches_and_two_fill_bytes_give_identical_outputs(sc):
    """The pile is summed with atomic adds: integer sums do not depend on their order.  A byte nobody writes would show under a fill."""
    name = "planted_CCCTAA_ONT"
    first = ac.run_case(sc.align_windows, name)
    for _ in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(first, ac.run_case(sc.align_windows, name)))
    try:
        for fill in (0x5A, 0xA5):
            sc.debug_option("poison", fill)
            assert all(np.array_equal(a, b) for a, b in zip(first, ac.run_case(sc.align_windows, name))), hex(fill)
            ac.assert_equal(ac.run_case(sc.align_windows, "hand"), "hand")      # (another shape in the same buffers)
    finally:
        sc.debug_option("poison", 0)
    ac.assert_equal(ac.run_case(sc.align_windows, name), name)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("kw,code,msg", ac.REFUSALS, ids=ac.REFUSAL_IDS)
def test_refusals(sc, kw, code, msg):
    """TPS_E_ARG = -3, TPS_E_CAPACITY = -5, with the emulation's words; a refused call writes nothing; the call without the fault
    succeeds."""
    def raw(codes, codes_len, length, n, ref_codes, ref_codes_len, ref_length, n_ref, ref, centre, span, stat, stat_len, cols, cols_len, pile_row, pile, n_pile,
            pile_len):
        return sc.lib.tps_window_align(sc._h, _p(codes), codes_len, _p(length), n, _p(ref_codes), ref_codes_len, _p(ref_length), n_ref, _p(ref), _p(centre), span,
                                       _p(stat), stat_len, _p(cols), cols_len, _p(pile_row), _p(pile), n_pile, pile_len)
    rc, stat, cols, pile = ac.refusal_call(raw, **kw)
    assert (rc, sc._err()) == (code, msg)
    assert (stat == 99).all() and (cols == 99).all() and (pile == 99).all()
    e_rc, e_msg = emu.window_align_raw(*_emu_args(kw))
    assert (e_rc, e_msg) == (code, msg)
    rc, stat, cols, pile = ac.refusal_call(raw)
    assert rc == 0 and stat[:, 5].tolist() == [0, hiplib.ALIGN_NONE] and (cols == hiplib.ALIGN_UNCOVERED).all() and (pile == 0).all()


def _emu_args(kw):
    got = []
    ac.refusal_call(lambda *args: got.append(args) or 0, **kw)
    return got[0]


def test_an_empty_call_clears_the_pile(sc):
    pile = np.full((2, 100, 13), 5, np.int32)
    rc = sc.lib.tps_window_align(sc._h, None, 0, None, 0, None, 21, None, 3, None, None, 100, None, 0, None, 0, _p(np.zeros(1, np.int32)), _p(pile), 2, pile.size)
    assert rc == 0 and (pile == 0).all()
