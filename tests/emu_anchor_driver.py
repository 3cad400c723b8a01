"""Test helper: builds and drives tests/emu/emu_anchor.cpp (host emulation of the window and offset kernels, csrc/tps_anchor.h), and
builds tests/emu/emu_anchor_main.cpp, the stand-alone program the sanitizers run."""
import ctypes as C

import numpy as np

import emu_build
from topsicle_amd import hiplib, variants

DEPS = emu_build.deps("emu_anchor.cpp", headers=("tps_anchor.h", "tps_ends.h", "tps_tract.h", "tps_device.h", "tps_wave.h", "tps_pack.h"))


def build():
    return emu_build.shared("libtps_emu_anchor.so", "emu_anchor.cpp", DEPS)


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    return emu_build.program("emu_anchor_main_asan", "emu_anchor_main.cpp", DEPS)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_anchor_last_error.restype = C.c_char_p
        _lib.emu_end_window.restype = C.c_int
        _lib.emu_window_offsets.restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def rows(span):
    """(dwords of a codes row, dwords of a keep row)"""
    return (span + 15) // 16, (span + 31) // 32


def end_window_code(seqs, code, m, tails, begin, end, k=12, span=2000, base_shift=0, lens=None):
    """end_window with the unit as the C ABI takes it (code, m): the refusals of a bad unit can be asked for.  `lens` = (n_reads,
    codes_len, keep_len) handed over, where they are not the right ones."""
    L = lib()
    bases, offsets = hiplib.pack_reads(seqs)
    n = len(seqs)
    tails = np.ascontiguousarray(tails, np.uint8)
    begin = np.ascontiguousarray(begin, np.int32)
    end = np.ascontiguousarray(end, np.int32)
    cdw, kdw = rows(span if 1 <= span <= hiplib.ANCHOR_MAX_SPAN else 1)
    codes = np.zeros((n, cdw), np.uint32)
    keep = np.zeros((n, kdw), np.uint32)
    nl, cl, kl = lens if lens is not None else (len(tails), codes.size, keep.size)
    rc = L.emu_end_window(_p(bases), _p(offsets), C.c_int64(n), C.c_uint64(code), m, k, _p(tails), _p(begin), _p(end), C.c_int64(nl), span, base_shift,
                          _p(codes), C.c_int64(cl), _p(keep), C.c_int64(kl))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_end_window rc={rc}: {L.emu_anchor_last_error().decode()}")
    return codes, keep


def end_window(seqs, unit, tails, begin, end, k=12, span=2000, base_shift=0):
    """(codes uint32[n, cdw], keep uint32[n, kdw]) like HipScanner.end_window; raises TopsicleHipError with the C ABI's return code in
    the message where tps_batch_end_window refuses."""
    code, m = variants.unit_code(unit)
    return end_window_code(seqs, code, m, tails, begin, end, k, span, base_shift)


def window_offsets(codes, keep, length, ref, span, k=12, n=None, out_len=None):
    """(offset, votes, second) int32[n] like HipScanner.anchor_offsets.  `n`, `out_len`: what is handed over where it is not what the
    arrays say."""
    L = lib()
    codes = np.ascontiguousarray(codes, np.uint32)
    keep = np.ascontiguousarray(keep, np.uint32)
    length = np.ascontiguousarray(length, np.int32)
    ref = np.ascontiguousarray(ref, np.int32)
    rows_n = len(ref)
    n = rows_n if n is None else n
    out_len = n if out_len is None else out_len
    offset, votes, second = (np.zeros(rows_n, np.int32) for _ in range(3))
    rc = L.emu_window_offsets(_p(codes), _p(keep), _p(length), _p(ref), C.c_int64(n), span, k, _p(offset), _p(votes), _p(second), C.c_int64(out_len))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_window_offsets rc={rc}: {L.emu_anchor_last_error().decode()}")
    return offset, votes, second
