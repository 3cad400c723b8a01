"""The `topsicle` command line on motifs of 16 to 32 letters against the reference's own main(): the runs tests/record_wide_cli.py
recorded (tests/golden/widecli_*.json) replayed on the emulated wide engines with the rules of
tests/test_ref_cli_differential.py (CSV row sequence, summary lines, filtered and raw-count files byte for byte, as digests),
and on the MI355X through the real CLI and the native reader -- one of them again from an unaligned BAM."""
import json
import os
import sys

import pytest

import cli_cases
import record_wide_cli as rec
import ref_import
from test_ref_cli_differential import compare_replayed, run_product
from topsicle_amd import hiplib, main as cli


def golden(gold_dir):
    """[(file name, recorded run, its case rebuilt from the seed)]; a case that no longer has the recorded digest is an error."""
    out = []
    for f in sorted(f for f in os.listdir(gold_dir) if f.startswith("widecli_") and f.endswith(".json")):
        g = json.load(open(os.path.join(gold_dir, f)))
        case = rec.make_case(f[len("widecli_"):-len(".json")])
        assert g["case_sha256"] == cli_cases.case_digest(case) and g["argv"] == case["argv"], "the case generator changed: re-record with tests/record_wide_cli.py"
        out.append((f, g, case))
    return out


@pytest.fixture
def wide_engine_factory():
    import emu_driver
    import emu_wide_driver
    emu_driver.build()
    emu_wide_driver.build()
    from emu_wide_engine import EmuWideEngine
    return lambda: [EmuWideEngine(), EmuWideEngine()]


def test_recorded_runs_are_what_the_issue_asks_for(gold_dir):
    runs = golden(gold_dir)
    assert [f for f, _, _ in runs] == sorted(f"widecli_{n}.json" for n in rec.RUNS) and len(runs) >= 5
    for f, g, case in runs:
        assert os.path.getsize(os.path.join(gold_dir, f)) <= rec.MAX_BYTES and len(g["expected"]["csv"]) - 1 >= rec.MIN_ROWS, f
        motif, argv = case["argv"][1], case["argv"]
        ks = [int(x) for x in argv[argv.index("--telophrase") + 1:][:2]] if "--telophrase" in argv else [len(motif) - 2]
        assert 16 <= len(motif) <= 32 and any(hiplib.needs_wide(["A" * k] * min(2 * len(motif), 4 ** k)) for k in ks)
    assert {len(case["argv"][1]) for _, _, case in runs} == {16, 23, 25, 32}


def test_wide_cli_golden_cases(gold_dir, tmp_path, wide_engine_factory):
    for f, g, case in golden(gold_dir):
        inp, out = cli_cases.materialise(case, str(tmp_path / f))
        code = run_product(wide_engine_factory(), ["-i", inp, "-o", out] + case["argv"])
        assert code == case["exit"], f
        compare_replayed(g["expected"], cli_cases.normalise(out), f)


def test_a_motif_of_more_than_32_letters_ends_before_any_file_is_read(tmp_path, wide_engine_factory):
    out = tmp_path / "out"
    code = run_product(wide_engine_factory(), ["-i", str(tmp_path / "does_not_exist.fastq"), "-o", str(out), "--pattern", "ACGGATGTCTAACTTCTTGGTGTACGGATTTGA"])
    assert code == 2 and not os.path.exists(out / "telolengths_all.csv")


@pytest.mark.skipif(not os.path.isdir(ref_import.REFERENCE_ROOT), reason="the reference checkout is not on this machine")
def test_recording_is_reproducible(gold_dir):
    name = "m23_fa_gz"
    text, rows = rec.record(name)
    assert rows >= rec.MIN_ROWS and text == open(os.path.join(gold_dir, f"widecli_{name}.json")).read()


@pytest.mark.gpu
def test_wide_cli_golden_cases_on_gpu(gold_dir, tmp_path):
    for f, g, case in golden(gold_dir):
        inp, out = cli_cases.materialise(case, str(tmp_path / f))
        try:
            cli.main(["-i", inp, "-o", out] + case["argv"])
            code = None
        except SystemExit as e:
            code = e.code if e.code is not None else 0
        assert code == case["exit"], f
        compare_replayed(g["expected"], cli_cases.normalise(out), f)


@pytest.mark.gpu
def test_wide_cli_from_an_unaligned_bam_on_gpu(gold_dir, tmp_path):
    """The FASTQ run of the 16-letter motif at k = 4 and 14 again, its records as a uBAM: the same CSV rows and summary (the
    filtered files are named and formatted after the input, so they are not the recorded ones)."""
    import bam_tools as bt
    g = json.load(open(os.path.join(gold_dir, "widecli_m16_k4_k14.json")))
    case = rec.make_case("m16_k4_k14")
    inp, out = cli_cases.materialise(case, str(tmp_path / "ubam"))
    bam = os.path.join(os.path.dirname(inp), os.path.basename(inp).split(".")[0] + ".bam")
    lines = open(inp).read().split("\n")
    lines[1::4] = [ln.upper() for ln in lines[1::4]]      # (BAM has no lower case; both CLIs upper-case what they scan)
    with open(inp, "w") as h:
        h.write("\n".join(lines))
    bt.fastq_records_to_bam(inp, bam)
    os.remove(inp)
    cli.main(["-i", bam, "-o", out] + case["argv"])
    got = cli_cases.normalise(out)
    assert got["csv"] == g["expected"]["csv"] and got["summary"] == g["expected"]["summary"]
