"""Test helper: builds and drives tests/emu/emu_tract.cpp (host emulation of the tract map kernel, csrc/tps_tract.h), and builds
tests/emu/emu_tract_main.cpp, the stand-alone program the sanitizers run."""
import ctypes as C
import os
import subprocess

import numpy as np

from topsicle_amd import hiplib, variants

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_tract.cpp")
MAIN_SRC = os.path.join(HERE, "emu", "emu_tract_main.cpp")
DEPS = [SRC] + [os.path.join(HERE, "..", "topsicle_amd", "csrc", f) for f in ("tps_tract.h", "tps_device.h", "tps_wave.h", "tps_pack.h")] + \
       [os.path.join(HERE, "..", "include", "topsicle_hip.h")]
FLAGS = ["-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unknown-pragmas"]


def _fresh(out, deps):
    return os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)


def _compile(cmd, out):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = out + ".tmp%d" % os.getpid()
    subprocess.check_call(cmd + ["-o", tmp])
    os.replace(tmp, out)
    return out


def build():
    out = os.path.join(HERE, "emu", "_build", "libtps_emu_tract.so")
    if _fresh(out, DEPS):
        return out
    return _compile(["g++", "-O2"] + FLAGS + ["-shared", "-fPIC", SRC], out)


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    out = os.path.join(HERE, "emu", "_build", "emu_tract_main_asan")
    if _fresh(out, DEPS + [MAIN_SRC]):
        return out
    return _compile(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + FLAGS + [MAIN_SRC], out)


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
