"""`--adapters` on the host side: the flags, the batch pipeline's routes (one pass, two passes, several --telophrase on helper contexts),
the collector, the naming rule and the two files, with the kernels replaced by their host emulations (tests/emu_adapter_engine.py).
tests/test_gpu_adapter.py runs the same on the GPU."""
import csv
import os

import pytest

import adapter_cases as ac
from topsicle_amd import main as cli

IDENT, N_READS = ac.CLI_IDENT, ac.CLI_READS


@pytest.fixture(scope="module")
def engines():
    import emu_adapter_driver
    import emu_anchor_driver
    import emu_driver
    import emu_ends_driver
    import emu_follow_wide_driver
    import emu_motif_driver
    import emu_variant_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver, emu_variant_driver, emu_ends_driver, emu_anchor_driver,
              emu_adapter_driver):
        d.build()
    from emu_adapter_engine import EmuAdapterEngine
    return [EmuAdapterEngine(), EmuAdapterEngine()]


def _cli(argv, engines):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


def _read(path):
    return open(path, "rb").read()


def test_adapters_on_every_route(tmp_path, engines):
    d, fa = ac.write_cli_inputs(tmp_path)
    common = ["-i", d, "--pattern", "CCCTAA", "--minSeqLength", "1000", "--cutoff", "0.4"]
    _cli(common + ["-o", str(tmp_path / "plain")], engines)
    assert sum(len(getattr(e, "adapter_calls", [])) for e in engines) == 0                 # without the flag nothing is searched
    _cli(common + ["-o", str(tmp_path / "one"), "--adapters", fa, "--twopass", "off"], engines)
    _cli(common + ["-o", str(tmp_path / "two"), "--adapters", fa, "--twopass", "on"], engines)
    assert sum(len(getattr(e, "adapter_calls", [])) for e in engines) >= 2
    for f in ("adapters_4.csv", "adapter_summary_4.csv"):
        assert not os.path.exists(tmp_path / "plain" / f)
        assert _read(tmp_path / "one" / f) == _read(tmp_path / "two" / f)
    # every other output is the run's without --adapters, byte for byte (the log holds times and paths)
    others = sorted(f for f in os.listdir(tmp_path / "plain") if f != "topsicle_run.log")
    assert "telolengths_all.csv" in others
    for run in ("one", "two"):
        assert sorted(f for f in os.listdir(tmp_path / run) if f != "topsicle_run.log" and not f.startswith("adapter")) == others
        for f in others:
            assert _read(tmp_path / "plain" / f) == _read(tmp_path / run / f), f
    n_rows, named = ac.check_cli_outputs(str(tmp_path / "one"))
    n_planted_stored = n_rows - sum(1 for r in csv.DictReader(open(tmp_path / "one" / "adapters_4.csv")) if ac.detection_set(IDENT, N_READS)[3][int(r["readID"][4:])] < 0)
    print(f"--adapters on {N_READS} reads of {IDENT}: {n_rows} reads with a stored boundary, {n_planted_stored} of them with a planted adapter, {named} named")
    assert n_rows >= 30 and named >= 0.9 * n_planted_stored
    assert "scanned in two passes" in open(tmp_path / "two" / "topsicle_run.log").read()
    log = open(tmp_path / "one" / "topsicle_run.log").read()
    assert "adapters: 12 sequences" in log and "median adapter end of the named reads" in log


def test_adapters_with_several_telophrase_and_literal_sequences(tmp_path, engines):
    d, _fa = ac.write_cli_inputs(tmp_path)
    pats = ac.detection_set(IDENT, N_READS)[0]
    common = ["-i", d, "--pattern", "CCCTAACCCTAA", "--minSeqLength", "1000", "--cutoff", "0.4", "--telophrase", "4", "5"]
    _cli(common + ["-o", str(tmp_path / "plain")], engines)
    _cli(common + ["-o", str(tmp_path / "ad"), "--adapters"] + [p.lower() for p in pats], engines)
    assert _read(tmp_path / "plain" / "telolengths_all.csv") == _read(tmp_path / "ad" / "telolengths_all.csv")
    for k in (4, 5):
        rows = list(csv.DictReader(open(tmp_path / "ad" / f"adapters_{k}.csv")))
        planted = ac.detection_set(IDENT, N_READS)[3]
        assert len(rows) >= 30
        for r in rows:
            if r["adapter"]:
                assert r["adapter"] == f"adapter{planted[int(r['readID'][4:])] + 1}"
        assert sum(1 for r in rows if r["adapter"]) >= 20
    assert any(len(getattr(h, "adapter_calls", [])) for e in engines for h in getattr(e, "_helpers", []))       # (the helper contexts ran theirs)


def test_bad_adapter_flags_end_the_run_with_one_message(tmp_path, engines, capsys):
    d, fa = ac.write_cli_inputs(tmp_path)
    many = tmp_path / "many.fa"
    many.write_text("".join(f">a{j}\n{'ACGT' * 4}\n" for j in range(65)))
    for extra in (["--adapters", str(many)], ["--adapters", "ACGTACGTACG"], ["--adapters", "A" * 65], ["--adapters", "ACGTNACGTACGTACG"],
                  ["--adapters", fa, "--adaptersearch", "15"], ["--adapters", fa, "--adaptersearch", "1025"],
                  ["--adapters", fa, "--adaptersearch", "512", "--maxlengthtelo", "400"]):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            _cli(["-i", d, "-o", str(tmp_path / "out"), "--pattern", "CCCTAA", "--override"] + extra, engines)
        assert e.value.code == 2
        assert capsys.readouterr().out.count("--adapters needs") == 1
        assert not os.path.exists(tmp_path / "out" / "telolengths_all.csv")                 # before any file is read or written
