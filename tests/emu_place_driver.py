"""Test helper: builds and drives tests/emu/emu_place.cpp (host emulation of the placement kernel, csrc/tps_place.h), and builds
tests/emu/emu_place_main.cpp, the stand-alone program the sanitizers run."""
import ctypes as C

import numpy as np

import emu_build
from topsicle_amd import hiplib

DEPS = emu_build.deps("emu_place.cpp", headers=("tps_place.h", "tps_anchor.h", "tps_ends.h", "tps_tract.h", "tps_device.h", "tps_wave.h"))


def build():
    return emu_build.shared("libtps_emu_place.so", "emu_place.cpp", DEPS)


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    return emu_build.program("emu_place_main_asan", "emu_place_main.cpp", DEPS)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_place_last_error.restype = C.c_char_p
        _lib.emu_window_place.restype = C.c_int
        _lib.emu_place_dir_bits.restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def dir_bits():
    """The bits of the directory the last place_windows call built."""
    return lib().emu_place_dir_bits()


def place_windows(codes, keep, length, ref_codes, ref_keep, ref_length, span, k=12, max_occ=16, lens=None):
    """(ref, total, runner_ref, runner, offset, votes, second) int32[n] like HipScanner.place_windows; raises TopsicleHipError with the
    C ABI's return code in the message where tps_window_place refuses.  `lens` = (codes_len, keep_len, n, ref_codes_len, ref_keep_len,
    n_ref, out_len) handed over, where they are not what the arrays say."""
    L = lib()
    codes = np.ascontiguousarray(codes, np.uint32)
    keep = np.ascontiguousarray(keep, np.uint32)
    length = np.ascontiguousarray(length, np.int32)
    ref_codes = np.ascontiguousarray(ref_codes, np.uint32)
    ref_keep = np.ascontiguousarray(ref_keep, np.uint32)
    ref_length = np.ascontiguousarray(ref_length, np.int32)
    n, n_ref = len(length), len(ref_length)
    cl, kl, nn, rcl, rkl, nr, ol = lens if lens is not None else (codes.size, keep.size, n, ref_codes.size, ref_keep.size, n_ref, n)
    outs = np.zeros((7, n), np.int32)
    rc = L.emu_window_place(_p(codes), C.c_int64(cl), _p(keep), C.c_int64(kl), _p(length), C.c_int64(nn), _p(ref_codes), C.c_int64(rcl), _p(ref_keep),
                            C.c_int64(rkl), _p(ref_length), nr, span, k, max_occ, _p(outs), C.c_int64(ol))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_window_place rc={rc}: {L.emu_place_last_error().decode()}")
    return tuple(outs[j].copy() for j in range(7))
