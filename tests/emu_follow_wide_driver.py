"""Test helper: builds and drives tests/emu/emu_follow_wide.cpp (host emulation of the wide followers kernel, csrc/tps_wide.h)."""
import ctypes as C
import os

import numpy as np

import emu_build
from topsicle_amd import hiplib

DEPS = emu_build.deps("emu_follow_wide.cpp", headers=("tps_wide.h", "tps_wide_plan.h", "tps_device.h", "tps_wave.h", "tps_plan.h", "tps_pack.h"))


def build(asan=False):
    return emu_build.shared("libtps_emu_follow_wide_asan.so" if asan else "libtps_emu_follow_wide.so", "emu_follow_wide.cpp", DEPS, asan)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build(asan=bool(os.environ.get("TPS_EMU_ASAN"))))      # TPS_EMU_ASAN=1: the -fsanitize=address,undefined build
        _lib.emu_follow_wide_last_error.restype = C.c_char_p
        _lib.emu_followers_wide.restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def followers_wide(patterns, seqs, n_fwd, follow, lo=100, hi=2000, min_len=0, want_hist=True, base_shift=0):
    """(picks uint32[n, 2, n_fwd, pw], hist int64[2, n_fwd, 4**follow + 1] or None) like HipScanner.kmer_followers_wide; raises
    TopsicleHipError with the C ABI's return code in the message where tps_batch_kmer_followers_wide refuses."""
    L = lib()
    bases, offsets = hiplib.pack_reads(seqs)
    n, P, k = len(seqs), len(patterns), len(patterns[0])
    pw = max((hi - lo + 31) // 32, 1)
    picks = np.zeros((n, 2, max(n_fwd, 1), pw), np.uint32)
    # (asked for beyond 8 followers: a one-counter stand-in, so that the refusal is the kernel driver's own)
    hist = (np.zeros((2, max(n_fwd, 1), 4 ** follow + 1), np.uint64) if 0 <= follow <= 8 else np.zeros(1, np.uint64)) if want_hist else None
    rc = L.emu_followers_wide("".join(patterns).encode(), P, k, _p(bases), _p(offsets), C.c_int64(n), n_fwd, follow, lo, hi, min_len,
                              base_shift, _p(picks), C.c_int64(picks.size), _p(hist), C.c_int64(0 if hist is None else hist.size))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_followers_wide rc={rc}: {L.emu_follow_wide_last_error().decode()}")
    return picks, (None if hist is None else hist.astype(np.int64))
