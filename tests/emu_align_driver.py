"""Test helper: builds and drives tests/emu/emu_align.cpp (host emulation of the banded alignment kernel, csrc/tps_align.h), and
builds tests/emu/emu_align_main.cpp, the stand-alone program the sanitizers run."""
import ctypes as C

import numpy as np

import emu_build
from topsicle_amd import hiplib

DEPS = emu_build.deps("emu_align.cpp", headers=("tps_align.h", "tps_wave.h", "tps_pack.h"))


def build():
    return emu_build.shared("libtps_emu_align.so", "emu_align.cpp", DEPS)


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    return emu_build.program("emu_align_main_asan", "emu_align_main.cpp", DEPS)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_align_last_error.restype = C.c_char_p
        _lib.emu_window_align.restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def window_align_raw(codes, codes_len, length, n, ref_codes, ref_codes_len, ref_length, n_ref, ref, centre, span, stat, stat_len, cols, cols_len, pile_row, pile,
                     n_pile, pile_len):
    """The C call as it is, every length handed over as given: (rc, message)."""
    L = lib()
    rc = L.emu_window_align(_p(codes), C.c_int64(codes_len), _p(length), C.c_int64(n), _p(ref_codes), C.c_int64(ref_codes_len), _p(ref_length), C.c_int32(n_ref),
                            _p(ref), _p(centre), C.c_int32(span), _p(stat), C.c_int64(stat_len), _p(cols), C.c_int64(cols_len), _p(pile_row), _p(pile),
                            C.c_int32(n_pile), C.c_int64(pile_len))
    return rc, (L.emu_align_last_error().decode() if rc else "")


def window_align(codes, length, ref_codes, ref_length, ref, centre, span, cols=True, pile_row=None, n_pile=0):
    """(stat int32[n, 6], cols uint16[n, span] or None, pile int32[n_pile, span, 13] or None) like HipScanner.align_windows; raises
    TopsicleHipError with the C ABI's return code in the message where tps_window_align refuses."""
    codes = np.ascontiguousarray(codes, np.uint32)
    length = np.ascontiguousarray(length, np.int32)
    ref_codes = np.ascontiguousarray(ref_codes, np.uint32)
    ref_length = np.ascontiguousarray(ref_length, np.int32)
    ref = np.ascontiguousarray(ref, np.int32)
    centre = np.ascontiguousarray(centre, np.int32)
    pile_row = None if pile_row is None else np.ascontiguousarray(pile_row, np.int32)
    n, n_ref = len(length), len(ref_length)
    sp = span if 1 <= span <= hiplib.ALIGN_MAX_SPAN else 1
    stat = np.zeros((n, hiplib.ALIGN_STATS), np.int32)
    out_cols = np.zeros((n, sp), np.uint16) if cols else None
    pile = np.zeros((n_pile, sp, hiplib.ALIGN_PILE), np.int32) if n_pile > 0 else None
    rc, msg = window_align_raw(codes, codes.size, length, n, ref_codes, ref_codes.size, ref_length, n_ref, ref, centre, span, stat, stat.size, out_cols,
                               0 if out_cols is None else out_cols.size, pile_row, pile, n_pile, 0 if pile is None else pile.size)
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_window_align rc={rc}: {msg}")
    return stat, out_cols, pile
