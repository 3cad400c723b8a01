"""Test helper: builds and drives tests/emu/emu_refine.cpp (host emulation of the boundary refinement kernel, csrc/tps_refine.h), and
builds tests/emu/emu_refine_main.cpp, the stand-alone program the sanitizers run."""
import ctypes as C

import numpy as np

import emu_build
from topsicle_amd import hiplib, variants

DEPS = emu_build.deps("emu_refine.cpp", headers=("tps_refine.h", "tps_tract.h", "tps_device.h", "tps_wave.h", "tps_pack.h"))


def build():
    return emu_build.shared("libtps_emu_refine.so", "emu_refine.cpp", DEPS)


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    return emu_build.program("emu_refine_main_asan", "emu_refine_main.cpp", DEPS)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_refine_last_error.restype = C.c_char_p
        _lib.emu_boundary_refine.restype = C.c_int
    return _lib


def piece():
    """Positions of a staged piece: the kernel's own figure."""
    return int(lib().emu_refine_piece())


def wpg():
    return int(lib().emu_refine_wpg())


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def boundary_refine(seqs, unit, tails, begin, end, at, hit=2, miss=1, sep=200, base_shift=0, lens=None):
    """REFINE_DTYPE[n] like HipScanner.boundary_refine; raises TopsicleHipError with the C ABI's return code in the message where
    tps_batch_boundary_refine refuses.  `unit`: a string, or a (code, m) pair; `lens` = (n_reads, out_len) handed over, where they are
    not the right ones."""
    L = lib()
    bases, offsets = hiplib.pack_reads(seqs)
    n = len(seqs)
    code, m = unit if isinstance(unit, tuple) else variants.unit_code(unit)
    tails = np.ascontiguousarray(tails, np.uint8)
    begin = np.ascontiguousarray(begin, np.int32)
    end = np.ascontiguousarray(end, np.int32)
    at = np.ascontiguousarray(at, np.int32)
    out = np.zeros(n, hiplib.REFINE_DTYPE)
    nl, ol = lens if lens is not None else (len(tails), n)
    rc = L.emu_boundary_refine(_p(bases), _p(offsets), C.c_int64(n), C.c_uint64(code), m, _p(tails), _p(begin), _p(end), _p(at), C.c_int64(nl), hit, miss, sep,
                               base_shift, _p(out), C.c_int64(ol))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_boundary_refine rc={rc}: {L.emu_refine_last_error().decode()}")
    return out
