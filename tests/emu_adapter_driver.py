"""Test helper: builds and drives tests/emu/emu_adapter.cpp (host emulation of the adapter kernel, csrc/tps_adapter.h), and builds
tests/emu/emu_adapter_main.cpp, the stand-alone program the sanitizers run."""
import ctypes as C
import os

import numpy as np

from emu_ends_driver import FLAGS, _compile, _fresh
from topsicle_amd import adapters, hiplib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_adapter.cpp")
MAIN_SRC = os.path.join(HERE, "emu", "emu_adapter_main.cpp")
DEPS = [SRC] + [os.path.join(HERE, "..", "topsicle_amd", "csrc", f) for f in ("tps_adapter.h", "tps_device.h", "tps_wave.h", "tps_pack.h")] + \
       [os.path.join(HERE, "..", "include", "topsicle_hip.h")]


def build():
    out = os.path.join(HERE, "emu", "_build", "libtps_emu_adapter.so")
    if _fresh(out, DEPS):
        return out
    return _compile(["g++", "-O2"] + FLAGS + ["-shared", "-fPIC", SRC], out)


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    out = os.path.join(HERE, "emu", "_build", "emu_adapter_main_asan")
    if _fresh(out, DEPS + [MAIN_SRC]):
        return out
    return _compile(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + FLAGS + [MAIN_SRC], out)


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
