"""Test helper: builds and drives tests/emu/emu_motif.cpp (host emulation of the motif census kernel, csrc/tps_motif.h), and builds
tests/emu/emu_motif_main.cpp, the stand-alone program the sanitizers run."""
import ctypes as C

import numpy as np

import emu_build
from topsicle_amd import hiplib

DEPS = emu_build.deps("emu_motif.cpp", headers=("tps_motif.h", "tps_device.h", "tps_wave.h", "tps_pack.h"))


def build():
    return emu_build.shared("libtps_emu_motif.so", "emu_motif.cpp", DEPS)


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    return emu_build.program("emu_motif_main_asan", "emu_motif_main.cpp", DEPS)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_motif_last_error.restype = C.c_char_p
        _lib.emu_motif_census.restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def motif_census(seqs, u_min=4, u_max=32, lo=0, hi=1000, min_len=0, want_counts=False, base_shift=0):
    """(hits MOTIF_HIT_DTYPE[n, 2], counts int32[n, 2, u_max - u_min + 1] or None) like HipScanner.motif_census; raises
    TopsicleHipError with the C ABI's return code in the message where tps_batch_motif_census refuses."""
    L = lib()
    bases, offsets = hiplib.pack_reads(seqs)
    n = len(seqs)
    hits = np.zeros((n, 2), hiplib.MOTIF_HIT_DTYPE)
    counts = np.zeros((n, 2, max(u_max - u_min + 1, 0)), np.int32) if want_counts else None
    rc = L.emu_motif_census(_p(bases), _p(offsets), C.c_int64(n), u_min, u_max, lo, hi, min_len, base_shift, _p(hits), C.c_int64(hits.size),
                            _p(counts), C.c_int64(0 if counts is None else counts.size))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_motif_census rc={rc}: {L.emu_motif_last_error().decode()}")
    return hits, counts
