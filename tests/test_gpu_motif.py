"""The motif census on the GPU (tps_batch_motif_census, HipScanner.motif_census): equal to the plain restatement of the rule on the
edge cases and the ragged batch the emulation is checked on (tests/motif_cases.py); independent of the pattern table and of the scans
around it; and `--pattern auto` / `python -m topsicle_amd.motif` end to end."""
import csv
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_tools as bt
import motif_cases as mc
from topsicle_amd import allsteps, hiplib, motif, synth
from topsicle_amd import main as cli

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sc():
    with hiplib.HipScanner(0) as s:
        yield s


def test_census_before_any_table_and_every_case(sc):
    """The first thing this context does is a census: no tps_set_patterns has been called.  Then every case, with the counts."""
    assert getattr(sc, "patterns", None) in (None, [])
    for name, reads, kw in mc.cases():
        sc.upload(0, *hiplib.pack_reads(list(reads)))
        hits, counts = sc.motif_census(0, want_counts=True, **kw)
        mc.assert_equal(hits, counts, name)


@pytest.mark.parametrize("name", ["defaults", "ragged", "ragged_lo", "span4096_lo7", "u32_only", "n33", "min_len", "empty"])
def test_census_without_counts(sc, name):
    _, reads, kw = next(c for c in mc.cases() if c[0] == name)
    sc.upload(1, *hiplib.pack_reads(list(reads)))
    hits, counts = sc.motif_census(1, **kw)
    mc.assert_equal(hits, counts, name, with_counts=False)


@pytest.mark.parametrize("kw, code", [
    (dict(u_min=0), "error -3"), (dict(u_min=5, u_max=4), "error -3"), (dict(u_max=33), "error -3"),
    (dict(lo=-1), "error -5"), (dict(lo=10, hi=10), "error -5"), (dict(lo=0, hi=4097), "error -5"),
])
def test_refusals(sc, kw, code):
    sc.upload(2, *hiplib.pack_reads(["ACGT" * 100]))
    with pytest.raises(hiplib.TopsicleHipError) as e:
        sc.motif_census(2, **kw)
    assert code in str(e.value)


def test_census_between_two_scans_changes_nothing(sc):
    reads = list(mc.ragged())
    pats = allsteps.patterns_to_search(telopattern="CCCTAA", cut_length=4)
    sc.set_patterns(pats)
    sc.upload(4, *hiplib.pack_reads(reads))
    prm = hiplib.make_params(min_len=500, min_count=20, window=100, slide=6, trimfirst=100, maxlen=20000,
                             flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS | hiplib.F_STORE_RAW)

    def scan():
        sc.scan(4, prm)
        sc.sync()
        return sc.results(4), sc.window_sums(4), sc.window_raw(4), sc.batch_trc_counts(4)
    first = scan()
    hits, counts = sc.motif_census(4, want_counts=True)
    mc.assert_equal(hits, counts, "ragged")
    second = scan()
    assert first[0]["pass"].sum() > 10
    assert np.array_equal(first[0], second[0])
    for a, b in zip(first[1] + first[2] + first[3], second[1] + second[2] + second[3]):
        assert np.array_equal(a, b)


def _write_fasta(path, reads, gz=False):
    text = "".join(f">read{i}\n{s}\n" for i, s in enumerate(reads))
    with (gzip.open(path, "wt") if gz else open(path, "w")) as fh:
        fh.write(text)


def _cli(argv):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args)


@pytest.mark.parametrize("name", ["CCCTAA", "albicans23"])
def test_cli_pattern_auto(tmp_path, name):
    """--pattern auto finds the canonical motif and then IS the run with that motif: the same telolengths_all.csv, byte for byte."""
    want = motif.canonical(mc.MOTIFS[name])
    d = tmp_path / "in"
    d.mkdir()
    _write_fasta(str(d / "reads.fasta"), mc.vote_reads(name, synth.ONT))
    common = ["-i", str(d), "--minSeqLength", "5000", "--cutoff", "0.4", "--gpus", "1"]
    _cli(common + ["-o", str(tmp_path / "auto"), "--pattern", "auto"])
    _cli(common + ["-o", str(tmp_path / "given"), "--pattern", want])
    auto = open(tmp_path / "auto" / "telolengths_all.csv", "rb").read()
    assert auto == open(tmp_path / "given" / "telolengths_all.csv", "rb").read()
    assert len(auto.splitlines()) > 1                       # (not two empty tables)
    log = open(tmp_path / "auto" / "topsicle_run.log").read()
    assert f"--pattern auto: using {want} " in log
    k = len(want) - 2
    assert os.path.exists(tmp_path / "auto" / f"quadfit_{k}mer_{want}.png")


def test_cli_pattern_auto_ends_the_run_without_a_motif(tmp_path):
    rng = np.random.default_rng(1)
    d = tmp_path / "in"
    d.mkdir()
    _write_fasta(str(d / "noise.fasta"), ["".join("ACGT"[i] for i in rng.integers(0, 4, 6000)) for _ in range(40)] + ["CCCTAA" * 1000] * 2)
    with pytest.raises(SystemExit) as e:
        _cli(["-i", str(d), "-o", str(tmp_path / "out"), "--pattern", "auto", "--minSeqLength", "5000"])
    assert e.value.code == 2
    log = open(tmp_path / "out" / "topsicle_run.log").read()
    assert "--pattern auto found no motif" in log and "AACCCT" in log          # (2 read ends vote for it: fewer than 5)
    assert not os.path.exists(tmp_path / "out" / "telolengths_all.csv")


def test_motif_module_command_line(tmp_path):
    """python -m topsicle_amd.motif, as a process of its own: the table's first row, in the file and on the screen."""
    path = str(tmp_path / "reads.fasta.gz")
    _write_fasta(path, mc.vote_reads("AAACCCT", synth.ONT), gz=True)
    r = subprocess.run([sys.executable, "-m", "topsicle_amd.motif", "-i", path, "-o", str(tmp_path / "out"), "--minSeqLength", "5000", "--top", "3"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = list(csv.reader(open(tmp_path / "out" / "motif_census.csv")))
    assert rows[0] == ["rank", "motif", "period", "read_ends", "share", "total_support"]
    assert rows[1][:3] == ["1", "AAACCCT", "7"] and int(rows[1][3]) >= 90 and float(rows[1][4]) >= 0.9
    assert "--pattern AAACCCT" in r.stdout and "1     AAACCCT" in r.stdout


def test_find_motif_reads_bam_and_stops_at_max_reads(sc, tmp_path):
    """The census goes through the pipeline's own readers: a BAM of the reads gives the table their FASTA gives; max_reads stops it."""
    reads = mc.vote_reads("CCCTAA", synth.HIFI)
    fa, bam = str(tmp_path / "r.fasta"), str(tmp_path / "r.bam")
    _write_fasta(fa, reads)
    bt.write_bam(bam, [(f"read{i}", bt.FLAG_UNMAPPED, s, None, [], []) for i, s in enumerate(reads)])
    rows_fa, n_fa = motif.find_motif(fa, [sc], min_len=5000)
    rows_bam, n_bam = motif.find_motif(bam, [sc], min_len=5000)
    assert n_fa == n_bam == 200 and rows_fa == rows_bam and rows_fa[0][0] == "AACCCT"
    assert rows_fa == motif.tally(mc.motif_oracle.motif_census(reads, min_len=5000)[0])
    rows_50, n_50 = motif.find_motif(fa, [sc], min_len=5000, max_reads=50)
    assert n_50 == 50 and rows_50 == motif.tally(mc.motif_oracle.motif_census(reads[:50], min_len=5000)[0])
