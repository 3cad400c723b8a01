"""Test helper: builds and drives tests/emu/emu_lc_lds.cpp -- the host emulation of emu_scan.cpp as a library of its own whose
scans can run with PlanKnobs::lc_lds (the default kernels' candidate sums resident in LDS), with every emulation counter and the
planner's decision as the library's contexts get it."""
import contextlib
import ctypes as C

import numpy as np

import emu_build
import emu_driver as emu

DEPS = emu_build.deps("emu_lc_lds.cpp") + emu.DEPS

# counters (csrc/tps_wave.h)
EXACT_TOURNAMENTS, LANE_CANDS, ONE_LANE_FINISH, WAVE_FINISH, LDS_CANDS = 4, 7, 8, 9, 15

_lib = None


def build():
    return emu_build.shared("libtps_emu_lc_lds.so", "emu_lc_lds.cpp", DEPS)


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_last_error.restype = C.c_char_p
        _lib.emu_scan.restype = C.c_int
        _lib.emu_binseg.restype = C.c_int
        _lib.emu_plan_lc_lds.restype = C.c_int
    return _lib


def counters():
    L = lib()
    return np.array([L.emu_counter_ext(i) for i in range(16)], np.int64)


class _WithKnob:
    """The library as emu_driver sees it inside scanning(): emu_set_knobs, which emu_driver calls before every scan and which resets
    every planner knob, is followed by emu_set_lc_lds; everything else is the library's own."""

    def __init__(self, L, lc_lds):
        self._L, self._on = L, int(bool(lc_lds))

    def __getattr__(self, name):
        return getattr(self._L, name)

    def emu_set_knobs(self, *args):
        self._L.emu_set_knobs(*args)
        self._L.emu_set_lc_lds(self._on)


@contextlib.contextmanager
def scanning(lc_lds):
    """Scans of emu_driver run through THIS library inside the block, with PlanKnobs::lc_lds = lc_lds; yields a dict that holds the
    counters' increments once the block has ended."""
    got = {}
    L = lib()
    old, emu._lib = emu._lib, _WithKnob(L, lc_lds)
    before = counters()
    try:
        yield got
    finally:
        L.emu_set_lc_lds(0)
        emu._lib = old
        got.update(enumerate((counters() - before).tolist()))


def planned(patterns, prm, max_nwin, val_on=False):
    """What plan_geometry decides with the knobs of the library's contexts: dict(lc_lds, lc_cap, entries)."""
    out = (C.c_int32 * 3)()
    k = len(patterns[0])
    rc = lib().emu_plan_lc_lds("".join(patterns).encode(), len(patterns), k, C.byref(prm), C.c_int64(int(max_nwin)), int(bool(val_on)), out)
    if rc != 0:
        raise RuntimeError(lib().emu_last_error().decode())
    return dict(zip(["lc_lds", "lc_cap", "entries"], [int(x) for x in out]))
