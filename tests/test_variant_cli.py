"""`--variants` on the host side: the flags, the batch pipeline's three routes (one pass, two passes, several --telophrase on helper
contexts), the collectors and the files, with the kernels replaced by their host emulations (tests/emu_variant_engine.py).
tests/test_gpu_variant.py runs the same on the GPU."""
import os

import numpy as np
import pytest

import variant_cases as vc
from topsicle_amd import batch, hiplib, variants
from topsicle_amd import main as cli


@pytest.fixture(scope="module")
def engines():
    import emu_driver
    import emu_follow_wide_driver
    import emu_motif_driver
    import emu_variant_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver, emu_variant_driver):
        d.build()
    from emu_variant_engine import EmuVariantEngine
    return [EmuVariantEngine(), EmuVariantEngine()]


@pytest.fixture(scope="module")
def reads():
    return vc.cli_reads(40)


def _cli(argv, engines):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


def _read(path):
    return open(path, "rb").read()


def test_variants_on_every_route(tmp_path, engines, reads):
    d = tmp_path / "in"
    d.mkdir()
    vc.write_fasta(str(d / "reads.fasta"), reads)
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4"]
    _cli(common + ["-o", str(tmp_path / "plain")], engines)
    _cli(common + ["-o", str(tmp_path / "one"), "--variants", "--twopass", "off"], engines)
    _cli(common + ["-o", str(tmp_path / "two"), "--variants", "--twopass", "on"], engines)
    assert not os.path.exists(tmp_path / "plain" / "variants_4.csv")
    assert _read(tmp_path / "plain" / "telolengths_all.csv") == _read(tmp_path / "one" / "telolengths_all.csv") == _read(tmp_path / "two" / "telolengths_all.csv")
    for f in ("variants_4.csv", "variant_profile_4.csv"):
        assert _read(tmp_path / "one" / f) == _read(tmp_path / "two" / f)
    assert vc.check_cli_outputs(str(tmp_path / "one"), reads, "CCCTAA", [4]) >= 10
    assert "scanned in two passes" in open(tmp_path / "two" / "topsicle_run.log").read()
    log = open(tmp_path / "one" / "topsicle_run.log").read()
    assert "variant census of" in log and "canonical:" in log and "top classes:" in log


def test_variants_with_several_telophrase_and_small_bins(tmp_path, engines, reads):
    d = tmp_path / "in"
    d.mkdir()
    vc.write_fasta(str(d / "reads.fasta"), reads)
    common = ["-i", str(d), "--pattern", "CCCTAACCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--telophrase", "4", "5"]
    _cli(common + ["-o", str(tmp_path / "plain")], engines)
    _cli(common + ["-o", str(tmp_path / "var"), "--variants", "--variantbin", "64", "--variantbins", "7"], engines)
    assert _read(tmp_path / "plain" / "telolengths_all.csv") == _read(tmp_path / "var" / "telolengths_all.csv")
    assert vc.check_cli_outputs(str(tmp_path / "var"), reads, "CCCTAA", [4, 5], bin=64, n_bins=7) >= 20
    assert "is a power of CCCTAA" in open(tmp_path / "var" / "topsicle_run.log").read()
    assert any(len(getattr(h, "variant_calls", [])) for e in engines for h in getattr(e, "_helpers", []))        # (the helper contexts ran theirs)


def test_bad_variant_flags_end_the_run(tmp_path, engines, reads):
    d = tmp_path / "in"
    d.mkdir()
    vc.write_fasta(str(d / "reads.fasta"), reads[:4])
    for extra in (["--variantbin", "63"], ["--variantbins", "65"]):
        with pytest.raises(SystemExit) as e:
            _cli(["-i", str(d), "-o", str(tmp_path / "out"), "--pattern", "CCCTAA", "--variants", "--override"] + extra, engines)
        assert e.value.code == 2


def test_job_without_variants_is_untouched(engines, reads):
    """scan_jobs keeps returning 4-tuples, and a job with a spec returns the very same ones."""
    from topsicle_amd import allsteps
    pats = allsteps.patterns_to_search(telopattern="CCCTAA", cut_length=4)
    prm = hiplib.make_params(no_bp=1000, min_len=5000, min_count=100, window=100, slide=6, trimfirst=100, maxlen=20000)
    recs = [type("R", (), {"seq": s, "id": f"read{i}"})() for i, s in enumerate(reads[:20])]
    got = []
    spec = variants.VariantSpec("CCCTAA", 500, 40, sink=lambda *a: got.append(a))
    plain = batch.scan_jobs(engines[0], recs, [batch.Job(pats, prm)])
    with_spec = batch.scan_jobs(engines[0], recs, [batch.Job(pats, prm, variants=spec)])
    assert len(plain[0]) == len(with_spec[0]) == 4 and np.array_equal(plain[0][0], with_spec[0][0])
    (r, res, counts, profile), = got
    assert r is recs and counts.shape == (20, 26) and profile.shape == (40, 26) and counts[:, 0].sum() == profile[:, 0].sum() > 0
    begin, end = variants.tract_bounds(res, 100, 6, 20000)
    assert np.array_equal(counts[:, 0], np.maximum(end - begin - 5, 0))
