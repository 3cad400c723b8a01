"""The layout accumulator of the read-analysis calls (tps::Layout, csrc/tps_layout.h): tests/emu/layout_main.cpp, a program of its
own under -fsanitize=address,undefined, holds it to the offsets the library used to compute by hand -- for n in {0, 1, 15, 16, 17,
4097} reads and 1, 63 and 64 adapter patterns: the region layout, the adapter layout and every output layout, each piece aligned
as asked, no two overlapping, the total what the allocation was."""
import subprocess

import emu_build


def build_main():
    return emu_build.program("layout_main_asan", "layout_main.cpp", emu_build.deps(headers=("tps_layout.h",)))


def test_layouts_equal_the_hand_computed_offsets():
    out = subprocess.run([build_main()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok 18 layouts"), out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
