"""`--tracts` on the host side: the flags and the one-message exits, the batch pipeline (the map runs once per batch on the worker
that scanned it, on whole reads), the collector and the two files, with the kernels replaced by their host emulations
(tests/emu_tract_engine.py).  tests/test_gpu_tract.py runs the same on the GPU."""
import os

import numpy as np
import pytest

import tract_cases as tc
from topsicle_amd import batch, hiplib, tracts
from topsicle_amd import main as cli


@pytest.fixture(scope="module")
def engines():
    import emu_driver
    import emu_follow_wide_driver
    import emu_motif_driver
    import emu_tract_driver
    import emu_variant_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver, emu_variant_driver, emu_tract_driver):
        d.build()
    from emu_tract_engine import EmuTractEngine
    return [EmuTractEngine(), EmuTractEngine()]


@pytest.fixture(scope="module")
def reads():
    return tc.cli_reads(60)


def _cli(argv, engines):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


def _read(path):
    return open(path, "rb").read()


def _calls(engines):
    return sum(len(getattr(e, "tract_calls", [])) for e in engines) + \
        sum(len(getattr(h, "tract_calls", [])) for e in engines for h in getattr(e, "_helpers", []))


def test_tracts_files_classes_and_untouched_outputs(tmp_path, engines, reads):
    d = tmp_path / "in"
    d.mkdir()
    tc.write_fasta(str(d / "reads.fasta"), reads)
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4"]
    _cli(common + ["-o", str(tmp_path / "plain")], engines)
    _cli(common + ["-o", str(tmp_path / "off"), "--tracts", "--twopass", "off"], engines)
    _cli(common + ["-o", str(tmp_path / "on"), "--tracts", "--twopass", "on"], engines)
    assert not os.path.exists(tmp_path / "plain" / "tracts.csv") and not os.path.exists(tmp_path / "plain" / "tract_reads.csv")
    assert _read(tmp_path / "plain" / "telolengths_all.csv") == _read(tmp_path / "off" / "telolengths_all.csv") == _read(tmp_path / "on" / "telolengths_all.csv")
    for f in ("tracts.csv", "tract_reads.csv"):
        assert _read(tmp_path / "off" / f) == _read(tmp_path / "on" / f)
    classes = tc.check_cli_outputs(str(tmp_path / "off"), reads, "CCCTAA")
    for cls, idx in tc.PLANTED.items():
        assert [classes[i] for i in idx] == [cls] * len(idx)
    assert "terminal" in classes.values() and "none" in classes.values()
    log_on, log_off = open(tmp_path / "on" / "topsicle_run.log").read(), open(tmp_path / "off" / "topsicle_run.log").read()
    assert "--twopass on ignored" in log_on and "--twopass on ignored" not in log_off
    for log in (log_on, log_off):
        assert log.count("scanned as whole reads (--twopass off)") == 1 and "scanned in two passes" not in log
        assert "reads per class: fusion 10, both_ends 10, interstitial" in log and f"tract map of {len(reads)} reads" in log


def test_tracts_once_per_batch_with_variants_and_several_telophrase(tmp_path, engines, reads):
    d = tmp_path / "in"
    d.mkdir()
    tc.write_fasta(str(d / "reads.fasta"), reads)
    common = ["-i", str(d), "--pattern", "CCCTAACCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--telophrase", "4", "5", "--variants"]
    _cli(common + ["-o", str(tmp_path / "plain")], engines)
    before = _calls(engines)
    _cli(common + ["-o", str(tmp_path / "tr"), "--tracts", "--tractblock", "128", "--tractminhits", "40", "--tractgap", "0", "--tractminblocks", "1", "--tractedge", "300"], engines)
    assert _calls(engines) - before == 1                    # one batch, two k: one map
    for f in ("telolengths_all.csv", "variants_4.csv", "variants_5.csv", "variant_profile_4.csv", "variant_profile_5.csv"):
        assert _read(tmp_path / "plain" / f) == _read(tmp_path / "tr" / f)
    tc.check_cli_outputs(str(tmp_path / "tr"), reads, "CCCTAA", edge=300, block=128, min_hits=40, gap=0, min_blocks=1)
    assert "is a power of CCCTAA; the map looks for CCCTAA" in open(tmp_path / "tr" / "topsicle_run.log").read()


@pytest.mark.parametrize("extra", [["--tractblock", "96"], ["--tractblock", "2048"], ["--tractminhits", "0"], ["--tractminhits", "65"], ["--tractgap", "-1"],
                                   ["--tractgap", "65"], ["--tractminblocks", "0"], ["--tractminblocks", "65"], ["--tractedge", "-1"],
                                   ["--pattern", "CCT"], ["--pattern", "CACACA"]])
def test_bad_tract_flags_end_the_run_before_any_file_is_read(tmp_path, engines, extra):
    """One message, exit status 2, nothing read and nothing but the log written: the input directory does not even exist."""
    out = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        _cli(["-i", str(tmp_path / "no_such_dir"), "-o", str(out), "--pattern", "CCCTAA", "--tracts"] + extra, engines)
    assert e.value.code == 2 and os.listdir(out) == ["topsicle_run.log"]                  # (the log alone: it holds the message)
    assert open(out / "topsicle_run.log").read().count("--tracts needs") == 1


def test_flags_and_defaults():
    a = cli.build_parser().parse_args(["-i", "x", "-o", "y", "--pattern", "CCCTAA"])
    assert a.tracts is False and (a.tractblock, a.tractminhits, a.tractgap, a.tractminblocks, a.tractedge) == (64, 20, 1, 2, 256)
    assert (tracts.DEFAULT_BLOCK, tracts.DEFAULT_MIN_HITS, tracts.DEFAULT_GAP, tracts.DEFAULT_MIN_BLOCKS, tracts.DEFAULT_MAX_TRACTS) == (64, 20, 1, 2, 8)
    assert cli.build_parser().parse_args(["-i", "x", "-o", "y", "--pattern", "CCCTAA", "--tracts"]).tracts is True
    assert hiplib.TRACT_BLOCK_RANGE == (64, 1024) and hiplib.TRACT_MAX_TRACTS_RANGE == (1, 16) and hiplib.TRACT_UNIT_RANGE == (4, 32)
    assert hiplib.TRACT_DTYPE.names == ("begin", "end", "hits", "blocks")


def test_job_with_tracts_maps_every_read_and_changes_nothing(engines, reads):
    """scan_jobs keeps returning the same 4-tuples; the sink gets the map of the whole batch, passing reads or not; a batch in heads
    mode is refused."""
    from topsicle_amd import allsteps
    import tract_oracle
    pats = allsteps.patterns_to_search(telopattern="CCCTAA", cut_length=4)
    prm = hiplib.make_params(no_bp=1000, min_len=5000, min_count=100, window=100, slide=6, trimfirst=100, maxlen=20000)
    recs = [type("R", (), {"seq": s, "id": f"read{i}"})() for i, s in enumerate(reads[:24])]
    got = []
    spec = tracts.TractSpec("CCCTAA", sink=lambda *a: got.append(a))
    plain = batch.scan_jobs(engines[0], recs, [batch.Job(pats, prm)])
    with_spec = batch.scan_jobs(engines[0], recs, [batch.Job(pats, prm, tracts=spec)])
    assert len(plain[0]) == len(with_spec[0]) == 4 and np.array_equal(plain[0][0], with_spec[0][0])
    (r, t, found, totals), = got
    want = tract_oracle.tract_map(reads[:24], "CCCTAA")
    assert r is recs and np.array_equal(t, want[0]) and np.array_equal(found, want[1]) and np.array_equal(totals, want[2])
    assert (found[plain[0][0]["pass"] == 0].sum(axis=1) > 0).any()              # reads that did not pass step 1 have tracts too
    heads = type("B", (), {"full_len": [6000] * 24})()
    with pytest.raises(ValueError):
        batch.scan_jobs(engines[0], heads, [batch.Job(pats, prm, tracts=spec)])
