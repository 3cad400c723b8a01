"""`--ends` on the host side: the flags, the batch pipeline's three routes (one pass, two passes, several --telophrase on helper
contexts), the collector, the groups and the files, with the kernels replaced by their host emulations (tests/emu_ends_engine.py).
tests/test_gpu_ends.py runs the same on the GPU."""
import os

import numpy as np
import pytest

import ends_cases as ec
from topsicle_amd import batch, ends, hiplib
from topsicle_amd import main as cli

IDENT = "CCCTAA_ONT"


@pytest.fixture(scope="module")
def engines():
    import emu_driver
    import emu_ends_driver
    import emu_follow_wide_driver
    import emu_motif_driver
    import emu_variant_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver, emu_variant_driver, emu_ends_driver):
        d.build()
    from emu_ends_engine import EmuEndsEngine
    return [EmuEndsEngine(), EmuEndsEngine()]


@pytest.fixture(scope="module")
def reads():
    return ec.detection_reads(IDENT)[0]


def _cli(argv, engines):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


def _read(path):
    return open(path, "rb").read()


def test_ends_on_every_route(tmp_path, engines, reads):
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), reads)
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4"]
    calls = sum(len(getattr(e, "link_calls", [])) for e in engines)
    _cli(common + ["-o", str(tmp_path / "plain")], engines)
    _cli(common + ["-o", str(tmp_path / "one"), "--ends", "--twopass", "off"], engines)
    _cli(common + ["-o", str(tmp_path / "two"), "--ends", "--twopass", "on"], engines)
    assert not os.path.exists(tmp_path / "plain" / "end_reads_4.csv")
    assert _read(tmp_path / "plain" / "telolengths_all.csv") == _read(tmp_path / "one" / "telolengths_all.csv") == _read(tmp_path / "two" / "telolengths_all.csv")
    for f in ("end_reads_4.csv", "ends_4.csv"):
        assert _read(tmp_path / "one" / f) == _read(tmp_path / "two" / f)
    good = ec.check_cli_outputs(str(tmp_path / "one"), IDENT)
    print(f"--ends on {IDENT}: {good} of {ec.N_ENDS * ec.PER_END} planted reads in their end's group")
    assert good >= 0.9 * ec.N_ENDS * ec.PER_END
    assert "scanned in two passes" in open(tmp_path / "two" / "topsicle_run.log").read()
    log = open(tmp_path / "one" / "topsicle_run.log").read()
    assert "end groups against CCCTAA" in log and "reads assigned" in log and "their links were cut at" in log
    assert sum(len(getattr(e, "link_calls", [])) for e in engines) == calls + 2           # one link call per k and run


def test_ends_with_several_telophrase(tmp_path, engines, reads):
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), reads)
    common = ["-i", str(d), "--pattern", "CCCTAACCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--telophrase", "4", "5"]
    _cli(common + ["-o", str(tmp_path / "plain")], engines)
    _cli(common + ["-o", str(tmp_path / "ends"), "--ends"], engines)
    assert _read(tmp_path / "plain" / "telolengths_all.csv") == _read(tmp_path / "ends" / "telolengths_all.csv")
    assert ec.check_cli_outputs(str(tmp_path / "ends"), IDENT, [4, 5]) >= 0.9 * ec.N_ENDS * ec.PER_END
    assert "is a power of CCCTAA" in open(tmp_path / "ends" / "topsicle_run.log").read()
    assert any(len(getattr(h, "sketch_calls", [])) for e in engines for h in getattr(e, "_helpers", []))         # (the helper contexts ran theirs)


def test_bad_end_flags_end_the_run_with_one_message(tmp_path, engines, reads, capsys):
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), reads[:4])
    for pattern, extra in (("CCT", []), ("CCTCCT", []), ("CCCTAA", ["--endk", "7"]), ("CCCTAA", ["--endbuckets", "100"]), ("CCCTAA", ["--endminmatch", "0"]),
                           ("CCCTAA", ["--endspan", "16385"]), ("auto", ["--endk", "17"])):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            _cli(["-i", str(d), "-o", str(tmp_path / "out"), "--pattern", pattern, "--ends", "--override"] + extra, engines)
        assert e.value.code == 2
        assert capsys.readouterr().out.count("--ends needs") == 1
        assert not os.path.exists(tmp_path / "out" / "telolengths_all.csv")             # before any file is read or written


def test_job_without_ends_is_untouched(engines, reads):
    """scan_jobs keeps returning 4-tuples, and a job with a spec returns the very same ones."""
    from topsicle_amd import allsteps
    pats = allsteps.patterns_to_search(telopattern="CCCTAA", cut_length=4)
    prm = hiplib.make_params(no_bp=1000, min_len=5000, min_count=100, window=100, slide=6, trimfirst=100, maxlen=20000)
    recs = [type("R", (), {"seq": s, "id": f"read{i}"})() for i, s in enumerate(reads[:20])]
    got = []
    spec = ends.EndSpec("CCCTAA", sink=lambda *a: got.append(a))
    plain = batch.scan_jobs(engines[0], recs, [batch.Job(pats, prm)])
    with_spec = batch.scan_jobs(engines[0], recs, [batch.Job(pats, prm, ends=spec)])
    assert len(plain[0]) == len(with_spec[0]) == 4 and np.array_equal(plain[0][0], with_spec[0][0])
    (r, res, sketch, kept), = got
    begin, end = ends.windows(res, 100, 6, 20000, spec.span)
    assert r is recs and sketch.shape == (20, 256) and kept.shape == (20,) and ((kept > 0) == (end > begin)).all() and (kept > 0).sum() >= 10
    assert (sketch[kept == 0] == ends.EMPTY).all()
