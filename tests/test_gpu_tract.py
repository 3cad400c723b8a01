"""The tract map on the GPU (tps_batch_tract_map, HipScanner.tract_map), through the C ABI: equal to the plain restatement of the rule
on the cases the emulation is checked on (tests/tract_cases.py); independent of the pattern table and of the scans around it; the same
from launch to launch; one refusal per error the header lists; and `--tracts` end to end."""
import ctypes as C
import os

import numpy as np
import pytest

import tract_cases as tc
from topsicle_amd import allsteps, hiplib, variants
from topsicle_amd import main as cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    with hiplib.HipScanner(0) as s:
        yield s


def _map(sc, slot, c):
    sc.upload(slot, *hiplib.pack_reads(list(c.reads)))
    return sc.tract_map(slot, c.unit, **c.kw)


def test_map_before_any_table_and_every_case(sc):
    """The first thing this context does is a map: no tps_set_patterns has been called.  Then every case."""
    assert getattr(sc, "patterns", None) in (None, [])
    for c in tc.cases():
        got = _map(sc, 0, c)
        assert got[0].dtype == hiplib.TRACT_DTYPE and got[0].shape == (len(c.reads), 2, c.kw["max_tracts"])
        tc.assert_equal(got, c.name)


def test_map_between_two_scans_changes_nothing(sc):
    c = tc.ragged()
    pats = allsteps.patterns_to_search(telopattern="CCCTAA", cut_length=4)
    sc.set_patterns(pats)
    sc.upload(4, *hiplib.pack_reads(list(c.reads)))
    prm = hiplib.make_params(min_len=500, min_count=20, window=100, slide=6, trimfirst=100, maxlen=20000,
                             flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS | hiplib.F_STORE_RAW)

    def scan():
        sc.scan(4, prm)
        sc.sync()
        return sc.results(4), sc.window_sums(4), sc.window_raw(4), sc.batch_trc_counts(4)
    first = scan()
    tc.assert_equal(sc.tract_map(4, c.unit, **c.kw), "ragged")
    again = sc.results(4), sc.window_sums(4), sc.window_raw(4), sc.batch_trc_counts(4)           # as the scan left them
    second = scan()
    assert first[0]["pass"].sum() > 10
    for other in (again, second):
        assert np.array_equal(first[0], other[0])
        for a, b in zip(first[1] + first[2] + first[3], other[1] + other[2] + other[3]):
            assert np.array_equal(a, b)


def test_one_launch_repeated_gives_identical_outputs(sc):
    c = tc.ragged()
    first = _map(sc, 5, c)
    for _ in range(3):
        again = sc.tract_map(5, c.unit, **c.kw)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    tc.assert_equal(first, c.name)


def _raw_call(sc, slot, code, m, block, min_hits, gap, min_blocks, max_tracts, n=1, lens=None):
    mt = max_tracts if 1 <= max_tracts <= 64 else 1
    tracts = np.zeros((n, 2, mt), hiplib.TRACT_DTYPE)
    found = np.zeros((n, 2), np.int32)
    totals = np.zeros((n, 4), np.uint32)
    tl, fl, ol = lens if lens is not None else (n * 2 * max_tracts, found.size, totals.size)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    return sc.lib.tps_batch_tract_map(sc._h, slot, C.c_uint64(code), m, block, min_hits, gap, min_blocks, max_tracts, p(tracts), tl, p(found), fl, p(totals), ol)


@pytest.mark.parametrize("kw, code", [
    (dict(code=variants.unit_code("CCT")[0], m=3), -3), (dict(code=0, m=33), -3), (dict(code=variants.unit_code("CCACCA")[0]), -3),
    (dict(code=variants.unit_code("CCCTAA")[0] | 1 << 12), -3),
    (dict(lens=(15, 2, 4)), -3), (dict(lens=(16, 3, 4)), -3), (dict(lens=(16, 2, 5)), -3),
    (dict(block=0), -5), (dict(block=96), -5), (dict(block=1088), -5),
    (dict(min_hits=0), -5), (dict(min_hits=65), -5), (dict(gap=-1), -5), (dict(gap=65), -5),
    (dict(min_blocks=0), -5), (dict(min_blocks=65), -5), (dict(max_tracts=0, lens=(0, 2, 4)), -5), (dict(max_tracts=17, lens=(34, 2, 4)), -5),
    (dict(slot=9), -6),
])
def test_refusals(sc, kw, code):
    """TPS_E_ARG = -3, TPS_E_CAPACITY = -5, TPS_E_STATE = -6 (a slot nothing was uploaded to); the call with that one argument
    corrected succeeds."""
    sc.upload(3, *hiplib.pack_reads(["CCCTAA" * 20]))
    good = dict(slot=3, code=variants.unit_code("CCCTAA")[0], m=6, block=64, min_hits=20, gap=1, min_blocks=2, max_tracts=8)
    a = dict(good)
    a.update(kw)
    assert _raw_call(sc, **a) == code
    assert _raw_call(sc, **good) == 0                  # (and what it refuses it refuses for that reason alone)


def _cli(argv):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args)


def _read(path):
    return open(path, "rb").read()


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """200 synthetic 6000-base reads, 30 of them planted, through the CLI: without --tracts, with it on either --twopass, and beside
    --variants --telophrase 4 5."""
    tmp = tmp_path_factory.mktemp("tracts_cli")
    reads = tc.cli_reads(200)
    d = tmp / "in"
    d.mkdir()
    tc.write_fasta(str(d / "reads.fasta"), reads)
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--gpus", "1"]
    _cli(common + ["-o", str(tmp / "plain")])
    _cli(common + ["-o", str(tmp / "off"), "--tracts", "--twopass", "off"])
    _cli(common + ["-o", str(tmp / "on"), "--tracts", "--twopass", "on"])
    _cli(common + ["-o", str(tmp / "plain45"), "--variants", "--telophrase", "4", "5"])
    _cli(common + ["-o", str(tmp / "k45"), "--variants", "--telophrase", "4", "5", "--tracts"])
    return tmp, reads


def test_cli_files_equal_oracle_and_classify(cli_runs):
    tmp, reads = cli_runs
    classes = tc.check_cli_outputs(str(tmp / "off"), reads, "CCCTAA")
    for cls, idx in tc.PLANTED.items():
        assert [classes[i] for i in idx] == [cls] * len(idx)
    assert list(classes.values()).count("terminal") > 50 and list(classes.values()).count("none") > 50
    tc.check_cli_outputs(str(tmp / "k45"), reads, "CCCTAA")


def test_cli_twopass_on_writes_the_same_files_and_says_so(cli_runs):
    tmp, reads = cli_runs
    for f in ("tracts.csv", "tract_reads.csv"):
        assert _read(tmp / "off" / f) == _read(tmp / "on" / f)
    log_on, log_off = open(tmp / "on" / "topsicle_run.log").read(), open(tmp / "off" / "topsicle_run.log").read()
    assert "--twopass on ignored" in log_on and "--twopass on ignored" not in log_off
    assert "scanned in two passes" not in log_on and "reads per class: fusion 10, both_ends 10, interstitial" in log_on


def test_cli_existing_outputs_do_not_change(cli_runs):
    tmp, reads = cli_runs
    assert not os.path.exists(tmp / "plain" / "tracts.csv") and not os.path.exists(tmp / "plain" / "tract_reads.csv")
    assert _read(tmp / "plain" / "telolengths_all.csv") == _read(tmp / "off" / "telolengths_all.csv") == _read(tmp / "on" / "telolengths_all.csv")
    for f in ("telolengths_all.csv", "variants_4.csv", "variants_5.csv", "variant_profile_4.csv", "variant_profile_5.csv"):
        assert _read(tmp / "plain45" / f) == _read(tmp / "k45" / f)
    assert len(_read(tmp / "plain" / "telolengths_all.csv").splitlines()) > 60
