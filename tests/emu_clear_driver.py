"""Test helper: builds tests/emu/emu_clear_main.cpp, the stand-alone program the sanitizers run over the host rule for reads that do
not pass (tps::clear_skipped_windows and tps::widen_sums16 of csrc/tps_plan.h)."""
import emu_build

DEPS = emu_build.deps("emu_clear_main.cpp", headers=("tps_plan.h", "tps_device.h", "tps_wave.h"))


def build_main():
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined."""
    return emu_build.program("emu_clear_main_asan", "emu_clear_main.cpp", DEPS)
