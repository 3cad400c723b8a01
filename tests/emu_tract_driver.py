"""Test helper: builds and drives tests/emu/emu_tract.cpp (host emulation of the tract map kernel, csrc/tps_tract.h), and builds
tests/emu/emu_tract_main.cpp, the stand-alone program the sanitizers run."""
import ctypes as C

import numpy as np

import emu_build
from topsicle_amd import hiplib, variants

DEPS = emu_build.deps("emu_tract.cpp", headers=("tps_tract.h", "tps_device.h", "tps_wave.h", "tps_pack.h"))


def build():
    return emu_build.shared("libtps_emu_tract.so", "emu_tract.cpp", DEPS)


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    return emu_build.program("emu_tract_main_asan", "emu_tract_main.cpp", DEPS)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_tract_last_error.restype = C.c_char_p
        _lib.emu_tract_map.restype = C.c_int
        _lib.emu_tract_table.restype = C.c_int
        _lib.emu_tract_piece.restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def piece(block):
    """Positions of one staged piece of the kernel's walk through a read, for this block size."""
    return int(lib().emu_tract_piece(int(block)))


def hit_table(unit):
    """The hit table the library's host code builds for `unit`: uint32[4^w / 16], entry c in bits [2 (c % 16), +1] of word c / 16."""
    code, m = variants.unit_code(unit)
    tab = np.zeros(4 ** min(m, 8) // 16, np.uint32)
    assert lib().emu_tract_table(C.c_uint64(code), m, _p(tab)) == 0
    return tab


def tract_map_code(seqs, code, m, block=64, min_hits=20, gap=1, min_blocks=2, max_tracts=8, base_shift=0, lens=None):
    """tract_map with the unit as the C ABI takes it (code, m): the refusals of a bad unit can be asked for.  `lens` = the three
    array lengths handed over, where they are not the right ones."""
    L = lib()
    bases, offsets = hiplib.pack_reads(seqs)
    n = len(seqs)
    mt = max_tracts if 1 <= max_tracts <= 64 else 1
    tracts = np.zeros((n, 2, mt), hiplib.TRACT_DTYPE)
    found = np.zeros((n, 2), np.int32)
    totals = np.zeros((n, 4), np.uint32)
    tl, fl, ol = lens if lens is not None else (n * 2 * max_tracts, found.size, totals.size)
    rc = L.emu_tract_map(_p(bases), _p(offsets), C.c_int64(n), C.c_uint64(code), m, block, min_hits, gap, min_blocks, max_tracts, base_shift,
                         _p(tracts), C.c_int64(tl), _p(found), C.c_int64(fl), _p(totals), C.c_int64(ol))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_tract_map rc={rc}: {L.emu_tract_last_error().decode()}")
    return tracts, found, totals


def tract_map(seqs, unit, block=64, min_hits=20, gap=1, min_blocks=2, max_tracts=8, base_shift=0):
    """(tracts[n, 2, max_tracts], found int32[n, 2], totals uint32[n, 4]) like HipScanner.tract_map; raises TopsicleHipError with
    the C ABI's return code in the message where tps_batch_tract_map refuses."""
    code, m = variants.unit_code(unit)
    return tract_map_code(seqs, code, m, block, min_hits, gap, min_blocks, max_tracts, base_shift)
