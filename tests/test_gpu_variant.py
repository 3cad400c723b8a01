"""The variant census on the GPU (tps_batch_variant_census, HipScanner.variant_census): equal to the plain restatement of the rule on
the cases the emulation is checked on (tests/variant_cases.py); independent of the pattern table and of the scans around it; the same
from launch to launch; and `--variants` end to end on the one-pass route, the two-pass route and several --telophrase."""
import ctypes as C
import os

import numpy as np
import pytest

import variant_cases as vc
from topsicle_amd import allsteps, hiplib, variants
from topsicle_amd import main as cli

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sc():
    with hiplib.HipScanner(0) as s:
        yield s


def _census(sc, slot, c, **kw):
    sc.upload(slot, *hiplib.pack_reads(list(c.reads)))
    reads, unit, tails, begin, end = c.args()
    return sc.variant_census(slot, unit, tails, begin, end, **c.kw(), **kw)


def test_census_before_any_table_and_every_case(sc):
    """The first thing this context does is a census: no tps_set_patterns has been called.  Then every case, with the profile."""
    assert getattr(sc, "patterns", None) in (None, [])
    for c in vc.cases():
        counts, profile = _census(sc, 0, c)
        vc.assert_equal(counts, profile, c.name)


@pytest.mark.parametrize("name", ["lengths_AAAC", "lengths_m32", "straddle_albicans23", "letters_glabrata16", "ragged", "long_m32_bin4064", "empty"])
def test_census_without_profile(sc, name):
    counts, profile = _census(sc, 1, vc.case(name), want_profile=False)
    vc.assert_equal(counts, profile, name, with_profile=False)


@pytest.mark.parametrize("unit, place, letter, name", vc.ISOLATED)
@pytest.mark.parametrize("tail", [0, 1])
def test_isolated_variants_count_m_each(sc, unit, place, letter, name, tail):
    """Independent of the oracle: each planted unit adds exactly m to its class and takes m from canonical."""
    m, planted = len(unit), 7
    read, begin, end = vc.isolated(unit, place, letter, planted, tail)
    sc.upload(2, *hiplib.pack_reads([read]))
    counts, profile = sc.variant_census(2, unit, [tail], [begin], [end])
    n, canon, other, cls = variants.split_row(counts[0], unit)
    assert n == end - m + 1 and other == 0 and canon == n - m * planted
    assert dict(zip(variants.class_names(unit), cls))[name] == m * planted and sum(cls) == m * planted
    assert np.array_equal(profile.sum(axis=0), counts[0].astype(np.int64))


def _raw_call(sc, slot, code, m, tails, begin, end, bin, n_bins, n_reads=None, counts_len=None, profile_len=None):
    tails, begin, end = np.array(tails, np.uint8), np.array(begin, np.int32), np.array(end, np.int32)
    cols = 2 + 4 * max(m, 0)
    counts = np.zeros((len(tails), cols), np.uint32)
    profile = np.zeros((max(n_bins, 0), cols), np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    return sc.lib.tps_batch_variant_census(sc._h, slot, C.c_uint64(code), m, p(tails), p(begin), p(end), len(tails) if n_reads is None else n_reads, bin, n_bins,
                                           p(counts), counts.size if counts_len is None else counts_len, p(profile), profile.size if profile_len is None else profile_len)


@pytest.mark.parametrize("kw, code", [
    (dict(code=0b0110, m=1), -3), (dict(code=0, m=33), -3), (dict(code=variants.unit_code("CCACCA")[0]), -3), (dict(code=variants.unit_code("AA")[0], m=2), -3),
    (dict(code=1 << 12), -3),
    (dict(begin=[-1]), -3), (dict(begin=[-2], end=[-1]), -3), (dict(begin=[5], end=[4]), -3), (dict(tails=[2]), -3),
    (dict(tails=[0, 0], begin=[0, 0], end=[1, 1]), -3), (dict(counts_len=25), -3), (dict(profile_len=26 * 39), -3),
    (dict(bin=63), -5), (dict(bin=4065), -5), (dict(n_bins=0), -5), (dict(n_bins=65), -5),
    (dict(slot=9), -6),
])
def test_refusals(sc, kw, code):
    """TPS_E_ARG = -3, TPS_E_CAPACITY = -5, TPS_E_STATE = -6 (a slot nothing was uploaded to)."""
    sc.upload(3, *hiplib.pack_reads(["CCCTAA" * 20]))
    a = dict(slot=3, code=variants.unit_code("CCCTAA")[0], m=6, tails=[0], begin=[0], end=[100], bin=500, n_bins=40)
    a.update(kw)
    assert _raw_call(sc, **a) == code
    a = dict(slot=3, code=variants.unit_code("CCCTAA")[0], m=6, tails=[0], begin=[0], end=[100], bin=500, n_bins=40)
    assert _raw_call(sc, **a) == 0                  # (and what it refuses it refuses for that reason alone)


def test_census_between_two_scans_changes_nothing(sc):
    c = vc.ragged()
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
    reads, unit, tails, begin, end = c.args()
    counts, profile = sc.variant_census(4, unit, tails, begin, end, **c.kw())
    vc.assert_equal(counts, profile, "ragged")
    again = sc.results(4), sc.window_sums(4), sc.window_raw(4), sc.batch_trc_counts(4)           # as the scan left them
    second = scan()
    assert first[0]["pass"].sum() > 10
    for other in (again, second):
        assert np.array_equal(first[0], other[0])
        for a, b in zip(first[1] + first[2] + first[3], other[1] + other[2] + other[3]):
            assert np.array_equal(a, b)


def test_one_launch_repeated_gives_identical_outputs(sc):
    c = vc.case("long_CCCTAA_bin64")
    first = _census(sc, 5, c)
    reads, unit, tails, begin, end = c.args()
    for _ in range(3):
        counts, profile = sc.variant_census(5, unit, tails, begin, end, **c.kw())
        assert np.array_equal(counts, first[0]) and np.array_equal(profile, first[1])
    vc.assert_equal(first[0], first[1], c.name)


def _cli(argv):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args)


def _read(path):
    return open(path, "rb").read()


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """~200 synthetic 6000-base ONT reads through the CLI: without --variants, one pass, two passes, and --telophrase 4 5."""
    tmp = tmp_path_factory.mktemp("variants_cli")
    reads = vc.cli_reads(200)
    d = tmp / "in"
    d.mkdir()
    vc.write_fasta(str(d / "reads.fasta"), reads)
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--gpus", "1"]
    _cli(common + ["-o", str(tmp / "plain")])
    _cli(common + ["-o", str(tmp / "one"), "--variants", "--twopass", "off"])
    _cli(common + ["-o", str(tmp / "two"), "--variants", "--twopass", "on"])
    _cli(common + ["-o", str(tmp / "plain45"), "--telophrase", "4", "5"])
    _cli(common + ["-o", str(tmp / "k45"), "--variants", "--telophrase", "4", "5"])
    return tmp, reads


def test_cli_both_routes_write_the_same_files(cli_runs):
    tmp, reads = cli_runs
    for f in ("variants_4.csv", "variant_profile_4.csv"):
        assert _read(tmp / "one" / f) == _read(tmp / "two" / f)
    assert "scanned in two passes" in open(tmp / "two" / "topsicle_run.log").read()
    assert "scanned in two passes" not in open(tmp / "one" / "topsicle_run.log").read()
    log = open(tmp / "one" / "topsicle_run.log").read()
    assert "variant census of" in log and "canonical:" in log and "top classes:" in log


def test_cli_rows_equal_the_oracle(cli_runs):
    tmp, reads = cli_runs
    assert vc.check_cli_outputs(str(tmp / "one"), reads, "CCCTAA", [4]) >= 60
    assert vc.check_cli_outputs(str(tmp / "k45"), reads, "CCCTAA", [4, 5]) >= 120


def test_cli_telolengths_do_not_change(cli_runs):
    tmp, reads = cli_runs
    assert not os.path.exists(tmp / "plain" / "variants_4.csv")
    assert _read(tmp / "plain" / "telolengths_all.csv") == _read(tmp / "one" / "telolengths_all.csv") == _read(tmp / "two" / "telolengths_all.csv")
    assert _read(tmp / "plain45" / "telolengths_all.csv") == _read(tmp / "k45" / "telolengths_all.csv")
    assert len(_read(tmp / "plain" / "telolengths_all.csv").splitlines()) > 60
