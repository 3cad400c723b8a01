"""AddressSanitizer + UndefinedBehaviorSanitizer over the host emulation of the wide-table scan kernel (csrc/tps_wide.h,
tests/emu/emu_wide.cpp): the case matrix of tests/test_wide_tables.py again on the -fsanitize=address,undefined build, in a child
interpreter with libasan preloaded.  A wave's LDS slice is allocated at exactly its planned size there, so every index past the
plan -- staged bases, position bytes, lane counters, the walk's state -- is an error, as is one past the result arrays."""
import os
import sys

from test_sanitizers import ROOT, _run_under_sanitizers


def test_wide_kernel_emulation_under_asan_ubsan():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import emu_driver
    import emu_wide_driver
    emu_driver.build(asan=True)
    emu_wide_driver.build(asan=True)
    out = _run_under_sanitizers(["tests/test_wide_tables.py", "-k", "emulation_matches or hash_tables or both_emulations or limits"], {"TPS_EMU_ASAN": "1"})
    assert " passed" in out and "skipped" not in out.split("passed")[-1]
