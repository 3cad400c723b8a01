"""Test helper: builds and drives tests/emu/emu_variant.cpp (host emulation of the variant census kernel, csrc/tps_variant.h), and
builds tests/emu/emu_variant_main.cpp, the stand-alone program the sanitizers run."""
import ctypes as C

import numpy as np

import emu_build
from topsicle_amd import hiplib, variants

DEPS = emu_build.deps("emu_variant.cpp", headers=("tps_variant.h", "tps_device.h", "tps_wave.h", "tps_pack.h"))


def build():
    return emu_build.shared("libtps_emu_variant.so", "emu_variant.cpp", DEPS)


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    return emu_build.program("emu_variant_main_asan", "emu_variant_main.cpp", DEPS)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_variant_last_error.restype = C.c_char_p
        _lib.emu_variant_census.restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def variant_census_code(seqs, code, m, tails, begin, end, bin=500, n_bins=40, want_profile=True, base_shift=0):
    """variant_census with the unit as the C ABI takes it (code, m): the refusals of a bad unit can be asked for."""
    L = lib()
    bases, offsets = hiplib.pack_reads(seqs)
    n = len(seqs)
    tails = np.ascontiguousarray(tails, np.uint8)
    begin = np.ascontiguousarray(begin, np.int32)
    end = np.ascontiguousarray(end, np.int32)
    cols = 2 + 4 * max(m, 0)
    counts = np.zeros((n, cols), np.uint32)
    profile = np.zeros((max(n_bins, 0), cols), np.int64) if want_profile else None
    rc = L.emu_variant_census(_p(bases), _p(offsets), C.c_int64(n), C.c_uint64(code), m, _p(tails), _p(begin), _p(end), C.c_int64(len(tails)),
                              bin, n_bins, base_shift, _p(counts), C.c_int64(counts.size), _p(profile), C.c_int64(0 if profile is None else profile.size))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_variant_census rc={rc}: {L.emu_variant_last_error().decode()}")
    return counts, profile


def variant_census(seqs, unit, tails, begin, end, bin=500, n_bins=40, want_profile=True, base_shift=0):
    """(counts uint32[n, 2 + 4m], profile int64[n_bins, 2 + 4m] or None) like HipScanner.variant_census; raises TopsicleHipError
    with the C ABI's return code in the message where tps_batch_variant_census refuses."""
    code, m = variants.unit_code(unit)
    return variant_census_code(seqs, code, m, tails, begin, end, bin, n_bins, want_profile, base_shift)
