"""`--ends --endref` on the host side: the flags, the reference's pieces scanned like reads, the batch pipeline's routes (one pass, two
passes, several --telophrase on helper contexts, --pattern auto), the placement and the three files checked against the planted
truth, with the kernels replaced by their host emulations (tests/emu_place_engine.py).  tests/test_gpu_place.py runs the same on the
GPU."""
import os

import numpy as np
import pytest

import anchor_cases as ac
import ends_cases as ec
import place_cases as pc
from topsicle_amd import main as cli

NEW = ("ref_ends_", "named_reads_", "named_ends_")


@pytest.fixture(scope="module")
def engines():
    import emu_anchor_driver
    import emu_driver
    import emu_ends_driver
    import emu_follow_wide_driver
    import emu_motif_driver
    import emu_place_driver
    import emu_variant_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver, emu_variant_driver, emu_ends_driver, emu_anchor_driver, emu_place_driver):
        d.build()
    from emu_place_engine import EmuPlaceEngine
    return [EmuPlaceEngine(), EmuPlaceEngine()]


def _cli(argv, engines):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


def _read(path):
    return open(path, "rb").read()


def _inputs(tmp_path, ident, n_reads=None):
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), ec.detection_reads(ident)[0][:n_reads])
    pc.write_reference(str(tmp_path / "ref.fasta"), ident)         # (beside the input directory, not in it: it is no read file)
    return str(d), str(tmp_path / "ref.fasta")


def _calls(engines, what):
    return sum(len(getattr(e, what, [])) for e in engines)


@pytest.mark.parametrize("ident", ["CCCTAA_ONT", "CCCTAA_HIFI"])
def test_endref_on_every_route(tmp_path, engines, ident):
    d, ref = _inputs(tmp_path, ident)
    common = ["-i", d, "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--ends"]
    before = _calls(engines, "place_calls"), _calls(engines, "window_calls"), _calls(engines, "offset_calls")
    _cli(common + ["-o", str(tmp_path / "ends")], engines)
    assert (_calls(engines, "place_calls"), _calls(engines, "window_calls")) == before[:2]          # without the flag nothing is extracted or placed
    _cli(common + ["-o", str(tmp_path / "one"), "--endref", ref, "--twopass", "off"], engines)
    _cli(common + ["-o", str(tmp_path / "two"), "--endref", ref, "--twopass", "on"], engines)
    assert _calls(engines, "place_calls") == before[0] + 2 and _calls(engines, "offset_calls") == before[2]     # one call per k and run; no anchoring
    new = [f"{stem}4.csv" for stem in NEW]
    for f in new:
        assert not os.path.exists(tmp_path / "ends" / f) and _read(tmp_path / "one" / f) == _read(tmp_path / "two" / f)
    # every other output is the run's without --endref, byte for byte (the log holds times and paths); no anchored_* file without --anchor
    others = sorted(f for f in os.listdir(tmp_path / "ends") if f != "topsicle_run.log")
    assert "telolengths_all.csv" in others and "end_reads_4.csv" in others and "ends_4.csv" in others
    for run in ("one", "two"):
        assert sorted(f for f in os.listdir(tmp_path / run) if f != "topsicle_run.log" and f not in new) == others
        for f in others:
            assert _read(tmp_path / "ends" / f) == _read(tmp_path / run / f), f
    assert b"chr" not in _read(tmp_path / "one" / "telolengths_all.csv")                    # no reference row reaches it
    errors, n_named = pc.check_cli_outputs(str(tmp_path / "one"), ident)
    print(f"--ends --endref on {ident}: {n_named} reads named; error of ref_length against the planted length median / p95 / max "
          f"{np.median(errors):.0f} / {np.percentile(errors, 95):.0f} / {errors[-1]}")
    p95, worst = ac.BOUNDS[ident.rsplit("_", 1)[1]]
    assert np.percentile(errors, 95) <= p95 and errors[-1] <= worst
    assert "scanned in two passes" in open(tmp_path / "two" / "topsicle_run.log").read()
    log = open(tmp_path / "one" / "topsicle_run.log").read()
    assert "named ends: 6 of 6 reference pieces" in log and "placed reads named" in log and "end groups named, 0 with more than one name" in log
    assert "close runner-up" in log and "0 of them without a group" in log


def test_endref_beside_anchor_and_several_telophrase(tmp_path, engines):
    ident = "CCCTAA_ONT"
    d, ref = _inputs(tmp_path, ident)
    common = ["-i", d, "--pattern", "CCCTAACCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--telophrase", "4", "5", "--ends", "--anchor"]
    _cli(common + ["-o", str(tmp_path / "anchor")], engines)
    _cli(common + ["-o", str(tmp_path / "both"), "--endref", ref], engines)
    for k in (4, 5):
        for f in ("telolengths_all.csv", f"end_reads_{k}.csv", f"ends_{k}.csv", f"anchored_reads_{k}.csv", f"anchored_ends_{k}.csv"):
            assert _read(tmp_path / "anchor" / f) == _read(tmp_path / "both" / f)
        errors, n_named = pc.check_cli_outputs(str(tmp_path / "both"), ident, k)
        assert n_named >= 0.9 * pc.REF_ENDS * ec.PER_END and errors[-1] <= ac.BOUNDS["ONT"][1]
    assert any(len(getattr(h, "window_calls", [])) for e in engines for h in getattr(e, "_helpers", []))         # (the helper contexts ran theirs)


def test_endref_with_pattern_auto(tmp_path, engines):
    ident = "AAACCCT_HIFI"
    d, ref = _inputs(tmp_path, ident)
    _cli(["-i", d, "--pattern", "auto", "--minSeqLength", "5000", "--cutoff", "0.4", "--ends", "--endref", ref, "-o", str(tmp_path / "auto")], engines)
    k = len("AAACCCT") - 2
    errors, n_named = pc.check_cli_outputs(str(tmp_path / "auto"), ident, k)
    assert n_named >= 0.9 * pc.REF_ENDS * ec.PER_END and np.percentile(errors, 95) <= ac.BOUNDS["HIFI"][0] and errors[-1] <= ac.BOUNDS["HIFI"][1]


def test_gzipped_reference_of_subtelomeres_only(tmp_path, engines):
    """The reference as a gzip file whose records are shorter than maxlengthtelo: both pieces of a record are the record, and only the
    one whose side the telomere is on is an end."""
    import gzip
    ident = "CCCTAA_HIFI"
    d, _ref = _inputs(tmp_path, ident)
    records, truth = pc.detection_reference(ident)
    with gzip.open(tmp_path / "sub.fa.gz", "wt") as fh:
        for rid, seq in records:
            fh.write(f">{rid}h\n{seq[:6000]}\n>{rid}t\n{seq[-6000:]}\n")
    _cli(["-i", d, "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--ends", "--endref", str(tmp_path / "sub.fa.gz"),
          "-o", str(tmp_path / "out")], engines)
    refs = pc._rows(str(tmp_path / "out" / "ref_ends_4.csv"))[1:]
    assert [(r[0], r[9]) for r in refs[:4]] == [("chr1h_head", "1"), ("chr1h_tail", "0"), ("chr1t_head", "0"), ("chr1t_tail", "1")]
    assert sum(r[9] == "1" for r in refs) == 6 and all(r[3] == "6000" for r in refs)
    named = [r for r in pc._rows(str(tmp_path / "out" / "named_reads_4.csv"))[1:] if r[5] != ""]
    assert len(named) >= 0.9 * pc.REF_ENDS * ec.PER_END and {r[5] for r in named} == {"chr1h_head", "chr1t_tail", "chr2h_head", "chr2t_tail", "chr3h_head"}


def test_bad_endref_flags_end_the_run_with_one_message(tmp_path, engines, capsys):
    d, ref = _inputs(tmp_path, "CCCTAA_ONT", 4)
    for extra in (["--endref", ref], ["--endref", ref, "--ends", "--endspan", "5000"], ["--endref", ref, "--ends", "--endrefmaxocc", "0"],
                  ["--endref", ref, "--ends", "--endrefmaxocc", "65"], ["--endref", ref, "--ends", "--endrefminvotes", "0"]):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            _cli(["-i", d, "-o", str(tmp_path / "out"), "--pattern", "CCCTAA", "--override"] + extra, engines)
        assert e.value.code == 2
        assert capsys.readouterr().out.count("--endref needs") == 1
        assert not os.path.exists(tmp_path / "out" / "telolengths_all.csv")                 # before any file is read or written
