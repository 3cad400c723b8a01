"""Test helper: builds and drives tests/emu/emu_adapter.cpp (host emulation of the adapter kernel, csrc/tps_adapter.h), and builds
tests/emu/emu_adapter_main.cpp, the stand-alone program the sanitizers run."""
import ctypes as C

import numpy as np

import emu_build
from topsicle_amd import adapters, hiplib

DEPS = emu_build.deps("emu_adapter.cpp", headers=("tps_adapter.h", "tps_device.h", "tps_wave.h", "tps_pack.h"))


def build():
    return emu_build.shared("libtps_emu_adapter.so", "emu_adapter.cpp", DEPS)


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    return emu_build.program("emu_adapter_main_asan", "emu_adapter_main.cpp", DEPS)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_adapter_last_error.restype = C.c_char_p
        _lib.emu_adapter_find.restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def adapter_find(seqs, patterns, tails, begin, end, base_shift=0, lens=None):
    """(dist uint16[n, P], end uint16[n, P]) like HipScanner.adapter_find; raises TopsicleHipError with the C ABI's return code in the
    message where tps_batch_adapter_find refuses.  `patterns`: strings, or a (codes, lens) pair as adapters.pattern_codes gives it;
    `lens` = (n_reads, hits_len) handed over, where they are not the right ones."""
    L = lib()
    bases, offsets = hiplib.pack_reads(seqs)
    n = len(seqs)
    codes, plen = adapters.pattern_codes(patterns)
    P = len(plen)
    tails = np.ascontiguousarray(tails, np.uint8)
    begin = np.ascontiguousarray(begin, np.int32)
    end = np.ascontiguousarray(end, np.int32)
    hits = np.zeros((n, P, 2), np.uint16)
    nl, hl = lens if lens is not None else (len(tails), hits.size)
    rc = L.emu_adapter_find(_p(bases), _p(offsets), C.c_int64(n), _p(codes), _p(plen), P, _p(tails), _p(begin), _p(end), C.c_int64(nl), base_shift,
                            _p(hits), C.c_int64(hl))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_adapter_find rc={rc}: {L.emu_adapter_last_error().decode()}")
    return hits[:, :, 0].copy(), hits[:, :, 1].copy()
