"""`--ends --anchor --consensus` on the GPU, end to end through the CLI on the planted-end sets: the four files consistent with each
other and with the anchoring's, the same bytes in one pass and two, every other file as without the flag, every consensus within its
bar of the planted subtelomere; then `--endref` on the reference the run wrote names every group to its own record.  The twin of
tests/test_consensus_cli.py, which runs the host emulation."""
import os

import pytest

import consensus_cases as cc
import ends_cases as ec
from topsicle_amd import main as cli

pytestmark = pytest.mark.gpu


def _cli(argv):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args)


def _read(path):
    return open(path, "rb").read()


@pytest.mark.parametrize("ident", ["CCCTAA_ONT", "CCCTAA_HIFI"])
def test_cli_end_to_end_and_as_the_next_runs_reference(tmp_path, ident):
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), ec.detection_reads(ident)[0])
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", str(cc.MIN_SEQ), "--cutoff", "0.4", "--gpus", "1", "--ends"]
    _cli(common + ["--anchor", "-o", str(tmp_path / "anchor")])
    _cli(common + ["--anchor", "--consensus", "-o", str(tmp_path / "one"), "--twopass", "off"])
    _cli(common + ["--anchor", "--consensus", "-o", str(tmp_path / "two"), "--twopass", "on"])
    new = [f.format(k=4) for f in cc.NEW]
    for f in new:
        assert not os.path.exists(tmp_path / "anchor" / f) and _read(tmp_path / "one" / f) == _read(tmp_path / "two" / f), f
    others = sorted(f for f in os.listdir(tmp_path / "anchor") if f != "topsicle_run.log")
    assert "telolengths_all.csv" in others and "anchored_reads_4.csv" in others and "anchored_ends_4.csv" in others
    for run in ("one", "two"):
        assert sorted(f for f in os.listdir(tmp_path / run) if f != "topsicle_run.log" and f not in new) == others
        for f in others:
            assert _read(tmp_path / "anchor" / f) == _read(tmp_path / run / f), f
    edits = cc.check_cli_outputs(str(tmp_path / "one"), ident)
    print(f"--ends --anchor --consensus on {ident}: edits of the six consensus sequences in their planted subtelomeres {sorted(edits)}")
    log = open(tmp_path / "one" / "topsicle_run.log").read()
    assert "end consensus: 6 of 6 end groups have a consensus" in log and "0 touched the band's edge" in log and "will not serve" not in log
    _cli(common + ["--endref", str(tmp_path / "one" / "end_reference_4.fa"), "-o", str(tmp_path / "named")])
    cc.check_named_by_own_reference(str(tmp_path / "named"))
