"""`--ends --anchor` on the host side: the flags, the batch pipeline's routes (one pass, two passes, several --telophrase on helper
contexts), the collector's packed rows, the anchoring and the two files, with the kernels replaced by their host emulations
(tests/emu_anchor_engine.py).  tests/test_gpu_ends_anchor.py runs the same on the GPU."""
import os

import numpy as np
import pytest

import anchor_cases as ac
import ends_cases as ec
from topsicle_amd import main as cli

IDENT = "CCCTAA_ONT"


@pytest.fixture(scope="module")
def engines():
    import emu_anchor_driver
    import emu_driver
    import emu_ends_driver
    import emu_follow_wide_driver
    import emu_motif_driver
    import emu_variant_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver, emu_variant_driver, emu_ends_driver, emu_anchor_driver):
        d.build()
    from emu_anchor_engine import EmuAnchorEngine
    return [EmuAnchorEngine(), EmuAnchorEngine()]


@pytest.fixture(scope="module")
def reads():
    return ec.detection_reads(IDENT)[0]


def _cli(argv, engines):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


def _read(path):
    return open(path, "rb").read()


def test_anchor_on_every_route(tmp_path, engines, reads):
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), reads)
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4"]
    calls = sum(len(getattr(e, "offset_calls", [])) for e in engines)
    _cli(common + ["-o", str(tmp_path / "ends"), "--ends"], engines)
    assert sum(len(getattr(e, "window_calls", [])) for e in engines) == 0                  # without the flag nothing is extracted
    _cli(common + ["-o", str(tmp_path / "one"), "--ends", "--anchor", "--twopass", "off"], engines)
    _cli(common + ["-o", str(tmp_path / "two"), "--ends", "--anchor", "--twopass", "on"], engines)
    assert not os.path.exists(tmp_path / "ends" / "anchored_reads_4.csv") and not os.path.exists(tmp_path / "ends" / "anchored_ends_4.csv")
    for f in ("anchored_reads_4.csv", "anchored_ends_4.csv"):
        assert _read(tmp_path / "one" / f) == _read(tmp_path / "two" / f)
    # every other output is the run's without --anchor, byte for byte (the log holds times and paths)
    others = sorted(f for f in os.listdir(tmp_path / "ends") if f != "topsicle_run.log")
    assert "telolengths_all.csv" in others and "end_reads_4.csv" in others and "ends_4.csv" in others
    for run in ("one", "two"):
        assert sorted(f for f in os.listdir(tmp_path / run) if f != "topsicle_run.log" and not f.startswith("anchored_")) == others
        for f in others:
            assert _read(tmp_path / "ends" / f) == _read(tmp_path / run / f), f
    anchored_err, called_err, n_anchored = ac.check_cli_outputs(str(tmp_path / "one"), IDENT)
    print(f"--ends --anchor on {IDENT}: {n_anchored} reads anchored; pairwise error of anchored_length median / p95 / max "
          f"{np.median(anchored_err):.0f} / {np.percentile(anchored_err, 95):.0f} / {anchored_err[-1]}, of telo_length (the caller's own boundaries) "
          f"{np.median(called_err):.0f} / {np.percentile(called_err, 95):.0f} / {called_err[-1]}")
    p95, worst = ac.BOUNDS["ONT"]
    assert n_anchored >= 0.9 * ec.N_ENDS * ec.PER_END
    assert np.percentile(anchored_err, 95) <= p95 and anchored_err[-1] <= worst
    assert "scanned in two passes" in open(tmp_path / "two" / "topsicle_run.log").read()
    log = open(tmp_path / "one" / "topsicle_run.log").read()
    assert "anchored lengths: " in log and "grouped reads anchored" in log and "median |shift|" in log
    assert sum(len(getattr(e, "offset_calls", [])) for e in engines) == calls + 2          # one offsets call per k and run


def test_anchor_with_several_telophrase(tmp_path, engines, reads):
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), reads)
    common = ["-i", str(d), "--pattern", "CCCTAACCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--telophrase", "4", "5", "--ends"]
    _cli(common + ["-o", str(tmp_path / "ends")], engines)
    _cli(common + ["-o", str(tmp_path / "anchor"), "--anchor"], engines)
    for f in ("telolengths_all.csv", "end_reads_4.csv", "ends_4.csv", "end_reads_5.csv", "ends_5.csv"):
        assert _read(tmp_path / "ends" / f) == _read(tmp_path / "anchor" / f)
    for k in (4, 5):
        assert ac.check_cli_outputs(str(tmp_path / "anchor"), IDENT, k)[2] >= 0.9 * ec.N_ENDS * ec.PER_END
    assert any(len(getattr(h, "window_calls", [])) for e in engines for h in getattr(e, "_helpers", []))         # (the helper contexts ran theirs)


def test_anchor_with_pattern_auto(tmp_path, engines, reads):
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), reads)
    _cli(["-i", str(d), "--pattern", "auto", "--minSeqLength", "5000", "--cutoff", "0.4", "--ends", "--anchor", "-o", str(tmp_path / "auto")], engines)
    assert ac.check_cli_outputs(str(tmp_path / "auto"), IDENT)[2] >= 0.9 * ec.N_ENDS * ec.PER_END


def test_bad_anchor_flags_end_the_run_with_one_message(tmp_path, engines, reads, capsys):
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), reads[:4])
    for extra in (["--anchor"], ["--anchor", "--ends", "--endspan", "5000"], ["--anchor", "--ends", "--anchorminvotes", "0"]):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            _cli(["-i", str(d), "-o", str(tmp_path / "out"), "--pattern", "CCCTAA", "--override"] + extra, engines)
        assert e.value.code == 2
        assert capsys.readouterr().out.count("--anchor needs") == 1
        assert not os.path.exists(tmp_path / "out" / "telolengths_all.csv")                 # before any file is read or written
