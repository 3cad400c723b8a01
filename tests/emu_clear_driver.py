"""Test helper: builds tests/emu/emu_clear_main.cpp, the stand-alone program the sanitizers run over the host rule for reads that do
not pass (tps::clear_skipped_windows and tps::widen_sums16 of csrc/tps_plan.h)."""
import os

from emu_tract_driver import FLAGS, _compile, _fresh

HERE = os.path.dirname(os.path.abspath(__file__))
MAIN_SRC = os.path.join(HERE, "emu", "emu_clear_main.cpp")
DEPS = [MAIN_SRC] + [os.path.join(HERE, "..", "topsicle_amd", "csrc", f) for f in ("tps_plan.h", "tps_device.h", "tps_wave.h")] + \
       [os.path.join(HERE, "..", "include", "topsicle_hip.h")]


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    out = os.path.join(HERE, "emu", "_build", "emu_clear_main_asan")
    if _fresh(out, DEPS):
        return out
    return _compile(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + FLAGS + [MAIN_SRC], out)
