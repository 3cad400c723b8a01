"""Test helper: builds and drives tests/emu/emu_wide.cpp (host emulation of the wide-table scan kernel, csrc/tps_wide.h)."""
import ctypes as C
import os

import numpy as np

import emu_build
from topsicle_amd import hiplib

DEPS = emu_build.deps("emu_wide.cpp", headers=("tps_wide.h", "tps_wide_plan.h", "tps_device.h", "tps_wave.h", "tps_plan.h", "tps_pack.h"))


def build(asan=False):
    return emu_build.shared("libtps_emu_wide_asan.so" if asan else "libtps_emu_wide.so", "emu_wide.cpp", DEPS, asan)


def build_main():
    """tests/emu/emu_wide_main.cpp under -fsanitize=address,undefined: a program of its own, nothing loaded into Python."""
    return emu_build.program("emu_wide_main_asan", "emu_wide_main.cpp", DEPS)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build(asan=bool(os.environ.get("TPS_EMU_ASAN"))))      # TPS_EMU_ASAN=1: the -fsanitize=address,undefined build
        _lib.emu_wide_last_error.restype = C.c_char_p
        _lib.emu_wide_scan.restype = C.c_int
        _lib.emu_wide_table.restype = C.c_int
        _lib.emu_wide_plan.restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def table(patterns):
    """dict(n_groups, n_so, rot, mul, used, mask_lo, mask_hi) of the hash table tps_set_patterns_wide builds; raises like it."""
    out = np.zeros(8, np.uint32)
    rc = lib().emu_wide_table("".join(patterns).encode(), len(patterns), len(patterns[0]), _p(out))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_wide_table rc={rc}: {lib().emu_wide_last_error().decode()}")
    return dict(zip(["n_groups", "n_so", "rot", "mul", "used", "mask_lo", "mask_hi"], [int(x) for x in out[:7]]))


E_CAPACITY = -5                  # TPS_E_CAPACITY (include/topsicle_hip.h)
LDS_BUDGET = 160 * 1024          # what emu_wide_scan plans with: the MI355X's LDS per workgroup


def plan(patterns, prm, budget_bytes=LDS_BUDGET):
    """What plan_wide (csrc/tps_wide_plan.h) decides for a device whose workgroups may use `budget_bytes` of LDS:
    dict(tp_cap, tw, seq_dw, wpg, lds_bytes, n_so), or dict(error=TPS_E_*, message=...) where it refuses."""
    out = np.zeros(8, np.int64)
    L = lib()
    rc = L.emu_wide_plan("".join(patterns).encode(), len(patterns), len(patterns[0]), C.byref(prm), C.c_int64(budget_bytes), _p(out))
    if rc != 0:
        return dict(error=rc, message=L.emu_wide_last_error().decode())
    return dict(zip(["tp_cap", "tw", "seq_dw", "wpg", "lds_bytes", "n_so"], [int(x) for x in out[:6]]))


def scan(patterns, seqs, prm, tails=None, base_shift=0):
    """Returns dict(results, c_start, c_end, win_off, sums, raw) like emu_driver.scan."""
    L = lib()
    bases, offsets = hiplib.pack_reads(seqs)
    n, P, k = len(seqs), len(patterns), len(patterns[0])
    res = np.zeros(n, dtype=hiplib.RESULT_DTYPE)
    cs = np.zeros((n, P), np.int32)
    ce = np.zeros((n, P), np.int32)
    lens = np.diff(offsets)
    nw = [hiplib.window_count(int(x), prm.window, prm.slide, prm.trimfirst, prm.maxlen) for x in lens]
    tot = int(sum(nw))
    win_off = np.zeros(n + 1, np.int64)
    sums = np.zeros(max(tot, 1), np.int32)
    raw = np.zeros(max(tot * P, 1), np.uint8)
    t = None if tails is None else np.ascontiguousarray(tails, dtype=np.uint8)
    rc = L.emu_wide_scan("".join(patterns).encode(), P, k, _p(bases), _p(offsets), C.c_int64(n), _p(t), C.byref(prm),
                         base_shift, _p(res), _p(cs), _p(ce), _p(win_off), _p(sums), _p(raw))
    if rc != 0:
        raise hiplib.TopsicleHipError(f"emu_wide_scan rc={rc}: {L.emu_wide_last_error().decode()}")
    return dict(results=res, c_start=cs, c_end=ce, win_off=win_off, sums=sums[:tot], raw=raw[:tot * P].reshape(-1, P))
