"""Test helper: builds and drives tests/emu/emu_binseg.cpp -- the host emulation of emu_scan.cpp as a second library that also
exports every emulation counter (csrc/tps_wave.h: which change-point finish ran, crowded prefilters, the float64 D route) and a
scan that hands back the candidate-sum scratch blocks."""
import contextlib
import ctypes as C

import numpy as np

import emu_build
import emu_driver as emu
from topsicle_amd import hiplib

DEPS = emu_build.deps("emu_binseg.cpp") + emu.DEPS

# counters (csrc/tps_wave.h)
EXACT_TOURNAMENTS, LANE_CANDS, ONE_LANE_FINISH, WAVE_FINISH, CROWDED, F64_ROUTE = 4, 7, 8, 9, 10, 11

_lib = None


def build():
    return emu_build.shared("libtps_emu_binseg.so", "emu_binseg.cpp", DEPS)


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_last_error.restype = C.c_char_p
        _lib.emu_scan.restype = C.c_int
        _lib.emu_binseg.restype = C.c_int
        _lib.emu_scan_lc.restype = C.c_int
    return _lib


def counters():
    L = lib()
    return np.array([L.emu_counter_ext(i) for i in range(16)], np.int64)


@contextlib.contextmanager
def counting():
    """Scans of emu_driver (and of everything built on it, such as test_kernel_matrix.emu_scan) run through THIS library inside the
    block; yields a dict that holds the counters' increments once the block has ended."""
    got = {}
    old, emu._lib = emu._lib, lib()
    before = counters()
    try:
        yield got
    finally:
        emu._lib = old
        got.update(enumerate((counters() - before).tolist()))


def scan_lc(patterns, seqs, prm, lc_cap=0):
    """One scan through the default sums kernel of slide 6 (forward tails: run it without F_STEP1); dict(results, win_off, sums,
    lc = uint32[n, words] scratch blocks with 0xBEEFBEEF where nothing was stored, lc_cap).  lc_cap > 0: a smaller capacity of
    the blocks than the plan's."""
    L = lib()
    bases, offsets = hiplib.pack_reads(seqs)
    n, P, k = len(seqs), len(patterns), len(patterns[0])
    nw = [hiplib.window_count(int(x), prm.window, prm.slide, prm.trimfirst, prm.maxlen) for x in np.diff(offsets)]
    tot = int(sum(nw))
    words = max(nw) // prm.jump + 4
    res = np.zeros(n, dtype=hiplib.RESULT_DTYPE)
    win_off = np.zeros(n + 1, np.int64)
    sums = np.zeros(max(tot, 1), np.int32)
    lc = np.zeros((n, words), np.uint32)
    cap = C.c_int32(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L.emu_set_knobs(0, 0, 1)
    rc = L.emu_scan_lc("".join(patterns).encode(), P, k, p(bases), p(offsets), C.c_int64(n), C.byref(prm), int(lc_cap), p(res), p(win_off), p(sums),
                       p(lc), C.c_int64(words), C.byref(cap))
    L.emu_set_knobs(0, 0, 0)
    if rc != 0:
        raise RuntimeError(f"emu_scan_lc rc={rc}: {L.emu_last_error().decode()}")
    return dict(results=res, win_off=win_off, sums=sums[:tot], lc=lc, lc_cap=int(cap.value))
