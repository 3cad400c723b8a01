"""`--pattern auto` and `python -m topsicle_amd.motif` on the host side: the readers, the batch pipeline, the vote, the log and the
files, with the kernels replaced by their host emulations (tests/emu_motif_engine.py).  tests/test_gpu_motif.py runs the same on the GPU."""
import csv
import gzip
import os

import pytest

import bam_tools as bt
import motif_cases as mc
import motif_oracle
from topsicle_amd import main as cli
from topsicle_amd import motif, synth


@pytest.fixture(scope="module")
def engines():
    import emu_driver
    import emu_follow_wide_driver
    import emu_motif_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver):
        d.build()
    from emu_motif_engine import EmuMotifEngine
    return [EmuMotifEngine(), EmuMotifEngine()]


def _write_fasta(path, reads, gz=False):
    text = "".join(f">read{i}\n{s}\n" for i, s in enumerate(reads))
    with (gzip.open(path, "wt") if gz else open(path, "w")) as fh:
        fh.write(text)


def _cli(argv, engines):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


@pytest.fixture(scope="module")
def reads60():
    return mc.vote_reads("CCCTAA", synth.ONT)[:60]


def test_pattern_auto_is_the_run_with_the_found_motif(tmp_path, engines, reads60):
    d = tmp_path / "in"
    d.mkdir()
    _write_fasta(str(d / "reads.fasta"), reads60)
    common = ["-i", str(d), "--minSeqLength", "5000", "--cutoff", "0.4"]
    _cli(common + ["-o", str(tmp_path / "auto"), "--pattern", "auto"], engines)
    _cli(common + ["-o", str(tmp_path / "given"), "--pattern", "AACCCT"], engines)
    auto = open(tmp_path / "auto" / "telolengths_all.csv", "rb").read()
    assert auto == open(tmp_path / "given" / "telolengths_all.csv", "rb").read() and len(auto.splitlines()) > 1
    log = open(tmp_path / "auto" / "topsicle_run.log").read()
    assert "--pattern auto: using AACCCT " in log and "motif census of 60 reads" in log
    assert os.path.exists(tmp_path / "auto" / "quadfit_4mer_AACCCT.png")


def test_pattern_auto_ends_the_run_when_too_few_ends_agree(tmp_path, engines, reads60):
    telomeric = [r for r, h in zip(reads60, motif_oracle.motif_census(reads60)[0]) if h["support"].max() >= motif.MIN_SUPPORT]
    other = [r for r in reads60 if r not in telomeric]
    assert len(telomeric) >= 4 and len(other) >= 10
    for name, reads, said in (("few", telomeric[:4] + other, "only 4 read end(s) vote for the leading motif AACCCT"),
                              ("none", other, "no read end reaches the minimum support")):
        d = tmp_path / name
        d.mkdir()
        _write_fasta(str(d / "reads.fasta"), reads)
        with pytest.raises(SystemExit) as e:
            _cli(["-i", str(d), "-o", str(tmp_path / (name + "_out")), "--pattern", "auto", "--minSeqLength", "5000"], engines)
        assert e.value.code == 2
        log = open(tmp_path / (name + "_out") / "topsicle_run.log").read()
        assert "--pattern auto found no motif" in log and said in log
        assert not os.path.exists(tmp_path / (name + "_out") / "telolengths_all.csv")


def test_other_patterns_are_untouched(tmp_path, engines, reads60):
    """A motif given by hand never reaches the census (an engine without one serves it), `Auto` in any case does."""
    from emu_follow_wide_engine import EmuFollowWideEngine
    d = tmp_path / "in"
    d.mkdir()
    _write_fasta(str(d / "reads.fasta"), reads60[:20])
    _cli(["-i", str(d), "-o", str(tmp_path / "given"), "--pattern", "CCCTAA", "--minSeqLength", "5000"], [EmuFollowWideEngine()])
    assert "pattern auto" not in open(tmp_path / "given" / "topsicle_run.log").read()
    with pytest.raises(AttributeError):
        _cli(["-i", str(d), "-o", str(tmp_path / "auto"), "--pattern", "Auto", "--minSeqLength", "5000"], [EmuFollowWideEngine()])


def test_motif_command_line_and_every_reader(tmp_path, engines, reads60, capsys):
    """The module's own command line; FASTA, gzip'ed FASTA and BAM of the same reads give one table; --motifreads stops early."""
    fa, gz, bam = str(tmp_path / "r.fasta"), str(tmp_path / "r.fa.gz"), str(tmp_path / "r.bam")
    _write_fasta(fa, reads60)
    _write_fasta(gz, reads60, gz=True)
    bt.write_bam(bam, [(f"read{i}", bt.FLAG_UNMAPPED, s, None, [], []) for i, s in enumerate(reads60)])
    want = motif.tally(motif_oracle.motif_census(reads60, min_len=5000)[0])
    for path in (fa, gz, bam):
        assert motif.find_motif(path, engines, min_len=5000) == (want, 60)
    assert motif.find_motif(fa, engines, min_len=5000, max_reads=25) == (motif.tally(motif_oracle.motif_census(reads60[:25], min_len=5000)[0]), 25)
    assert motif.find_motif(fa, engines, min_len=6000) == ([], 60)              # every read is 6000 bases long: none is looked at
    rc = motif.main(["-i", fa, "-o", str(tmp_path / "out"), "--minSeqLength", "5000", "--top", "2"], engines=engines)
    out = capsys.readouterr().out
    assert rc == 0 and "--pattern AACCCT" in out and "1     AACCCT" in out
    rows = list(csv.reader(open(tmp_path / "out" / "motif_census.csv")))
    assert rows[0] == ["rank", "motif", "period", "read_ends", "share", "total_support"]
    assert rows[1] == ["1", "AACCCT", "6", str(want[0][2]), "%.4f" % (want[0][2] / sum(r[2] for r in want)), str(want[0][3])]
    assert len(rows) == 1 + len(want)
    assert motif.main(["-i", fa, "-o", str(tmp_path / "out2"), "--minSeqLength", "6000"], engines=engines) == 1
