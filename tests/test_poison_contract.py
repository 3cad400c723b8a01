"""What the library hands out for bytes no kernel wrote, on the host: the seven-read batch of tests/poison_cases.py through the
emulation of the kernel source (which ends in the very host functions the library's downloads call, csrc/tps_plan.h:
widen_sums16, clear_skipped_windows), on the generic kernel and on the fused one whose 16-bit sums sit in a garbage-filled padded
buffer; and the stand-alone program that runs those functions under AddressSanitizer and UndefinedBehaviorSanitizer.  The MI355X half
is tests/test_gpu_poison.py, which holds the GPU to the same expected arrays."""
import subprocess

import numpy as np
import pytest

import emu_clear_driver
import emu_driver as emu
import poison_cases as pc


def _scan(prm, tails=None, force_generic=0):
    out = emu.scan(pc.PATTERNS, list(pc.reads()), prm, tails=tails, force_generic=force_generic)
    tot = int(out["win_off"][-1])
    assert len(out["sums"]) == tot and out["raw"].shape == (tot, pc.P)
    return out


def test_the_batch_is_what_it_says():
    reads, want = pc.reads(), pc.expected()
    assert [len(x) for x in reads] == [1106, 900, 3000, 0, 1220, 1001, 1340]
    assert want["passes"].tolist() == [1, 0, 0, 0, 1, 0, 1] and want["tail"][6] == 1 and want["tail"][0] == 0
    assert "N" in reads[4] and set("".join(reads)) <= set("ACGTN")
    nw = np.diff(want["win_off"])
    assert nw[1] > 0 and nw[2] > 0 and nw[5] > 0 and nw[3] == 0          # the skipped reads have windows in the layout, the empty one none
    assert pc.expected(True)["passes"].tolist() == [1, 0, 1, 1, 0, 1, 1]


@pytest.mark.parametrize("force_generic", [0, 1], ids=["fused", "generic"])
def test_step1_scan_hands_out_zeros_for_reads_that_do_not_pass(force_generic):
    pc.assert_contract(_scan(pc.params(), force_generic=force_generic), tag=f"force_generic={force_generic}")


@pytest.mark.parametrize("force_generic", [0, 1], ids=["fused", "generic"])
def test_tails_in_scan_hands_out_zeros_for_skipped_reads(force_generic):
    pc.assert_contract(_scan(pc.params_tails(), tails=pc.tails_in(), force_generic=force_generic), by_hand=True, tag=f"force_generic={force_generic}")


def test_fused_and_generic_agree_on_every_byte():
    a, b = _scan(pc.params()), _scan(pc.params(), force_generic=1)
    for key in ("results", "c_start", "c_end", "win_off", "sums", "raw"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_host_rule_is_clean_under_sanitizers():
    """tps::clear_skipped_windows and tps::widen_sums16 as a program of their own under -fsanitize=address,undefined: no read
    passes, all pass, alternating, a zero-window read between two skipped ones, the 16-bit padded layout; whole arrays and pieces
    that begin and end inside a read, every buffer allocated at exactly its size."""
    exe = emu_clear_driver.build_main()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok 9 batches"), out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
