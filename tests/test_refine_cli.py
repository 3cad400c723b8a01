"""`--refine` on the host side: the flags, the batch pipeline's routes (one pass, two passes, several --telophrase on helper contexts),
the collector, the class rule and the two files, with the kernels replaced by their host emulations (tests/emu_refine_engine.py).
tests/test_gpu_refine.py runs the same on the GPU."""
import os

import numpy as np
import pytest

import refine_cases as rc
import variant_cases as vc
from topsicle_amd import main as cli


@pytest.fixture(scope="module")
def engines():
    import emu_adapter_driver
    import emu_anchor_driver
    import emu_driver
    import emu_ends_driver
    import emu_follow_wide_driver
    import emu_motif_driver
    import emu_refine_driver
    import emu_variant_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver, emu_variant_driver, emu_ends_driver, emu_anchor_driver,
              emu_adapter_driver, emu_refine_driver):
        d.build()
    from emu_refine_engine import EmuRefineEngine
    return [EmuRefineEngine(), EmuRefineEngine()]


@pytest.fixture(scope="module")
def reads():
    return rc.cli_reads()


def _cli(argv, engines):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


def _read(path):
    return open(path, "rb").read()


def test_refine_on_every_route(tmp_path, engines, reads):
    seqs, planted = reads
    d = tmp_path / "in"
    d.mkdir()
    vc.write_fasta(str(d / "reads.fasta"), seqs)
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4"]
    _cli(common + ["-o", str(tmp_path / "plain")], engines)
    assert sum(len(getattr(e, "refine_calls", [])) for e in engines) == 0                  # without the flag nothing is refined
    _cli(common + ["-o", str(tmp_path / "one"), "--refine", "--twopass", "off"], engines)
    _cli(common + ["-o", str(tmp_path / "two"), "--refine", "--twopass", "on"], engines)
    assert sum(len(getattr(e, "refine_calls", [])) for e in engines) >= 2
    for f in ("refined_4.csv", "refine_summary_4.csv"):
        assert not os.path.exists(tmp_path / "plain" / f)
        assert _read(tmp_path / "one" / f) == _read(tmp_path / "two" / f)
    # every other output is the run's without --refine, byte for byte (the log holds times and paths)
    others = sorted(f for f in os.listdir(tmp_path / "plain") if f != "topsicle_run.log")
    assert "telolengths_all.csv" in others
    for run in ("one", "two"):
        assert sorted(f for f in os.listdir(tmp_path / run) if f != "topsicle_run.log" and not f.startswith("refine")) == others
        for f in others:
            assert _read(tmp_path / "plain" / f) == _read(tmp_path / run / f), f
    rows = rc.check_cli_outputs(str(tmp_path / "one"), seqs, "CCCTAA", [4])
    assert len(rows) >= 20
    truth = np.array([planted[int(r["readID"][4:])] for r in rows])
    shift = np.abs(np.array([int(r["shift"]) for r in rows]))
    called = np.abs(np.array([int(r["telo_length"]) for r in rows]) - truth)
    refined = np.abs(np.array([int(r["refined_length"]) for r in rows]) - truth)
    fig = lambda x: (float(np.median(x)), float(np.percentile(x, 95)), int(x.max()))      # noqa: E731
    print(f"--refine on {len(seqs)} reads: {len(rows)} rows; median / p95 / max of |shift| {fig(shift)}, of |telo_length - planted| {fig(called)}, "
          f"of |refined_length - planted| {fig(refined)}")
    assert all(r["class"] == "clean" for r in rows if planted[int(r["readID"][4:])] > 0)
    assert "scanned in two passes" in open(tmp_path / "two" / "topsicle_run.log").read()
    log = open(tmp_path / "one" / "topsicle_run.log").read()
    assert "refined boundaries:" in log and "no_telomere 0, open 0, ambiguous 0, clean" in log and "of the clean reads" in log


def test_refine_with_several_telophrase(tmp_path, engines, reads):
    seqs, _planted = reads
    d = tmp_path / "in"
    d.mkdir()
    vc.write_fasta(str(d / "reads.fasta"), seqs[:40])
    common = ["-i", str(d), "--pattern", "CCCTAACCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--telophrase", "4", "5"]
    _cli(common + ["-o", str(tmp_path / "plain")], engines)
    _cli(common + ["-o", str(tmp_path / "ref"), "--refine", "--refinesep", "150", "--refinehit", "3", "--refinemiss", "2", "--refineminmargin", "40"], engines)
    assert _read(tmp_path / "plain" / "telolengths_all.csv") == _read(tmp_path / "ref" / "telolengths_all.csv")
    assert len(rc.check_cli_outputs(str(tmp_path / "ref"), seqs, "CCCTAA", [4, 5], hit=3, miss=2, sep=150, minmargin=40)) >= 10
    assert "is a power of CCCTAA" in open(tmp_path / "ref" / "topsicle_run.log").read()
    assert any(len(getattr(h, "refine_calls", [])) for e in engines for h in getattr(e, "_helpers", []))        # (the helper contexts ran theirs)


def test_bad_refine_flags_end_the_run_with_one_message(tmp_path, engines, capsys):
    for extra in (["--refinehit", "0"], ["--refinehit", "17"], ["--refinemiss", "0"], ["--refinemiss", "17"], ["--refinesep", "0"], ["--refinesep", "65536"],
                  ["--refineminscore", "-1"], ["--maxlengthtelo", "70000"], ["--maxlengthtelo", "65637"], ["--pattern", "CCA"]):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            _cli(["-i", str(tmp_path / "no_such_input"), "-o", str(tmp_path / "out"), "--pattern", "CCCTAA", "--override", "--refine"] + extra, engines)
        assert e.value.code == 2
        assert capsys.readouterr().out.count("--refine needs") == 1
        assert not os.path.exists(tmp_path / "out" / "telolengths_all.csv")                 # before any file is read or written
