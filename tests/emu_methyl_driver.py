"""Test helper: builds and drives tests/emu/emu_methyl.cpp (host emulation of the base-modification kernel, csrc/tps_methyl.h), and
builds tests/emu/emu_methyl_main.cpp and tests/emu/mods_main.cpp, the stand-alone programs the sanitizers run."""
import ctypes as C
import os

import numpy as np

import emu_build
from topsicle_amd import hiplib

DEPS = emu_build.deps("emu_methyl.cpp", headers=("tps_methyl.h", "tps_wave.h", "tps_pack.h"))


def build():
    return emu_build.shared("libtps_emu_methyl.so", "emu_methyl.cpp", DEPS)


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    return emu_build.program("emu_methyl_main_asan", "emu_methyl_main.cpp", DEPS)


def build_mods_main():
    """The aux walk of the native reader (tps_bam_mods_spans, csrc/tps_mods.h) as a stand-alone program under the sanitizers."""
    csrc = os.path.join(emu_build.HERE, "..", "topsicle_amd", "csrc")
    return emu_build.program("mods_main_asan", "mods_main.cpp", [os.path.join(csrc, "tps_mods.h")])


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_methyl_last_error.restype = C.c_char_p
        _lib.emu_mod_profile.restype = C.c_int
    return _lib


def wpg():
    return int(lib().emu_methyl_wpg())


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def mod_profile(seqs, tails, begin, end, origin, mod_off, delta, prob, w=500, nb0=2, nb1=8, hi=205, lo=50, base_shift=0, lens=None):
    """(MOD_ROW_DTYPE[n], MOD_BIN_DTYPE[n, nb0 + nb1]) like HipScanner.mod_profile; raises TopsicleHipError with the C ABI's return
    code in the message where tps_batch_mod_profile refuses.  `lens` = (n_reads, n_mods, rows_len, bins_len) handed over, where they
    are not the right ones."""
    L = lib()
    bases, offsets = hiplib.pack_reads(seqs)
    n = len(seqs)
    tails = np.ascontiguousarray(tails, np.uint8)
    begin, end, origin = (np.ascontiguousarray(x, np.int32) for x in (begin, end, origin))
    mod_off = np.ascontiguousarray(mod_off, np.int64)
    delta = np.ascontiguousarray(delta, np.uint32)
    prob = np.ascontiguousarray(prob, np.uint8)
    nb = max(nb0 + nb1, 0)
    rows = np.zeros(n, hiplib.MOD_ROW_DTYPE)
    bins = np.zeros((n, nb), hiplib.MOD_BIN_DTYPE)
    nr, nm, rl, bl = lens if lens is not None else (len(tails), len(delta), n, n * nb)
    rc = L.emu_mod_profile(_p(bases), _p(offsets), C.c_int64(n), _p(tails), _p(begin), _p(end), _p(origin), C.c_int64(nr), _p(mod_off), _p(delta), _p(prob),
                           C.c_int64(nm), int(w), int(nb0), int(nb1), int(hi), int(lo), base_shift, _p(rows), C.c_int64(rl), _p(bins), C.c_int64(bl))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_mod_profile rc={rc}: {L.emu_methyl_last_error().decode()}")
    return rows, bins
