"""Test helper: builds and drives tests/emu/emu_ends.cpp (host emulation of the end sketch and link kernels, csrc/tps_ends.h), and
builds tests/emu/emu_ends_main.cpp, the stand-alone program the sanitizers run."""
import ctypes as C

import numpy as np

import emu_build
from topsicle_amd import hiplib, variants

DEPS = emu_build.deps("emu_ends.cpp", headers=("tps_ends.h", "tps_tract.h", "tps_device.h", "tps_wave.h", "tps_pack.h"))


def build():
    return emu_build.shared("libtps_emu_ends.so", "emu_ends.cpp", DEPS)


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    return emu_build.program("emu_ends_main_asan", "emu_ends_main.cpp", DEPS)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_ends_last_error.restype = C.c_char_p
        _lib.emu_end_sketch.restype = C.c_int
        _lib.emu_sketch_links.restype = C.c_int
        _lib.emu_ends_piece.restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def piece():
    """k-mer positions of one staged piece of the sketch kernel's walk through a window."""
    return int(lib().emu_ends_piece())


def end_sketch_code(seqs, code, m, tails, begin, end, k=12, buckets=256, base_shift=0, lens=None):
    """end_sketch with the unit as the C ABI takes it (code, m): the refusals of a bad unit can be asked for.  `lens` = (n_reads,
    sketch_len, kept_len) handed over, where they are not the right ones."""
    L = lib()
    bases, offsets = hiplib.pack_reads(seqs)
    n = len(seqs)
    tails = np.ascontiguousarray(tails, np.uint8)
    begin = np.ascontiguousarray(begin, np.int32)
    end = np.ascontiguousarray(end, np.int32)
    nb = buckets if buckets in hiplib.ENDS_BUCKETS else 64
    sketch = np.zeros((n, nb), np.uint32)
    kept = np.zeros(n, np.uint32)
    nl, sl, kl = lens if lens is not None else (len(tails), n * buckets, n)
    rc = L.emu_end_sketch(_p(bases), _p(offsets), C.c_int64(n), C.c_uint64(code), m, k, buckets, _p(tails), _p(begin), _p(end), C.c_int64(nl), base_shift,
                          _p(sketch), C.c_int64(sl), _p(kept), C.c_int64(kl))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_end_sketch rc={rc}: {L.emu_ends_last_error().decode()}")
    return sketch, kept


def end_sketch(seqs, unit, tails, begin, end, k=12, buckets=256, base_shift=0):
    """(sketch uint32[n, buckets], kept uint32[n]) like HipScanner.end_sketch; raises TopsicleHipError with the C ABI's return code in
    the message where tps_batch_end_sketch refuses."""
    code, m = variants.unit_code(unit)
    return end_sketch_code(seqs, code, m, tails, begin, end, k, buckets, base_shift)


def sketch_links(sketch, min_match=6, max_links=32, buckets=None, lens=None, n=None):
    """(degree int32[n], links int32[n, max_links], matches int32[n, max_links]) like HipScanner.sketch_links.  `buckets`, `lens` =
    (sketch_len, degree_len, links_len, matches_len), `n`: what is handed over where it is not what the arrays say."""
    L = lib()
    sketch = np.ascontiguousarray(sketch, np.uint32)
    n = sketch.shape[0] if n is None else n
    b = sketch.shape[1] if buckets is None else buckets
    ml = max_links if 1 <= max_links <= hiplib.LINKS_MAX_LINKS else 1
    degree = np.zeros(sketch.shape[0], np.int32)
    links = np.zeros((sketch.shape[0], ml), np.int32)
    matches = np.zeros((sketch.shape[0], ml), np.int32)
    sl, dl, ll, tl = lens if lens is not None else (n * b, n, n * max_links, n * max_links)
    rc = L.emu_sketch_links(_p(sketch), C.c_int64(n), b, C.c_int64(sl), min_match, max_links, _p(degree), C.c_int64(dl), _p(links), C.c_int64(ll),
                            _p(matches), C.c_int64(tl))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_sketch_links rc={rc}: {L.emu_ends_last_error().decode()}")
    return degree, links, matches
