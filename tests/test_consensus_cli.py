"""`--ends --anchor --consensus` on the host side: the flags, the batch pipeline's routes (one pass, two passes), the four files checked
against each other, against the anchoring's files and against the planted subtelomeres, and `--endref` on the reference the run wrote
-- with the kernels replaced by their host emulations (tests/emu_align_engine.py).  tests/test_gpu_consensus.py runs the same on the
GPU."""
import os

import pytest

import consensus_cases as cc
import ends_cases as ec
from topsicle_amd import main as cli


@pytest.fixture(scope="module")
def engines():
    import emu_align_driver
    import emu_anchor_driver
    import emu_driver
    import emu_ends_driver
    import emu_follow_wide_driver
    import emu_motif_driver
    import emu_place_driver
    import emu_variant_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver, emu_variant_driver, emu_ends_driver, emu_anchor_driver, emu_place_driver,
              emu_align_driver):
        d.build()
    from emu_align_engine import EmuAlignEngine
    return [EmuAlignEngine(), EmuAlignEngine()]


def _cli(argv, engines):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


def _read(path):
    return open(path, "rb").read()


def _calls(engines, what):
    return sum(len(getattr(e, what, [])) for e in engines)


@pytest.mark.parametrize("ident", ["CCCTAA_ONT", "CCCTAA_HIFI"])
def test_consensus_on_every_route_and_as_the_next_runs_reference(tmp_path, engines, ident):
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), ec.detection_reads(ident)[0])
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", str(cc.MIN_SEQ), "--cutoff", "0.4", "--ends"]
    before = _calls(engines, "align_calls")
    _cli(common + ["--anchor", "-o", str(tmp_path / "anchor")], engines)
    assert _calls(engines, "align_calls") == before                                         # without the flag nothing is aligned
    _cli(common + ["--anchor", "--consensus", "-o", str(tmp_path / "one"), "--twopass", "off"], engines)
    _cli(common + ["--anchor", "--consensus", "-o", str(tmp_path / "two"), "--twopass", "on"], engines)
    assert _calls(engines, "align_calls") == before + 4                                     # two calls per k and run
    new = [f.format(k=4) for f in cc.NEW]
    for f in new:
        assert not os.path.exists(tmp_path / "anchor" / f) and _read(tmp_path / "one" / f) == _read(tmp_path / "two" / f), f
    # every other output is the run's without --consensus, byte for byte (the log holds times and paths)
    others = sorted(f for f in os.listdir(tmp_path / "anchor") if f != "topsicle_run.log")
    assert "telolengths_all.csv" in others and "anchored_reads_4.csv" in others and "anchored_ends_4.csv" in others
    for run in ("one", "two"):
        assert sorted(f for f in os.listdir(tmp_path / run) if f != "topsicle_run.log" and f not in new) == others
        for f in others:
            assert _read(tmp_path / "anchor" / f) == _read(tmp_path / run / f), f
    edits = cc.check_cli_outputs(str(tmp_path / "one"), ident)
    print(f"--ends --anchor --consensus on {ident}: edits of the six consensus sequences in their planted subtelomeres {sorted(edits)}")
    assert "scanned in two passes" in open(tmp_path / "two" / "topsicle_run.log").read()
    log = open(tmp_path / "one" / "topsicle_run.log").read()
    assert "end consensus: 6 of 6 end groups have a consensus" in log and "0 touched the band's edge" in log and "will not serve" not in log
    # the next run: the same reads named against the reference this run wrote
    _cli(common + ["--endref", str(tmp_path / "one" / "end_reference_4.fa"), "-o", str(tmp_path / "named")], engines)
    cc.check_named_by_own_reference(str(tmp_path / "named"))


def test_bad_consensus_flags_end_the_run_with_one_message(tmp_path, engines, capsys):
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), ec.detection_reads("CCCTAA_ONT")[0][:4])
    for extra in (["--consensus"], ["--consensus", "--ends"], ["--consensus", "--anchor"], ["--consensus", "--ends", "--anchor", "--consensusmindepth", "0"]):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            _cli(["-i", str(d), "-o", str(tmp_path / "out"), "--pattern", "CCCTAA", "--override"] + extra, engines)
        assert e.value.code == 2
        assert capsys.readouterr().out.count(" needs ") == 1
        assert not os.path.exists(tmp_path / "out" / "telolengths_all.csv")                 # before any file is read or written
