"""End groups on the GPU (tps_batch_end_sketch, tps_sketch_links; HipScanner.end_sketch, HipScanner.sketch_links), through the C ABI:
equal to the plain restatement of the rules on the cases the emulation is checked on (tests/ends_cases.py); independent of the
pattern table and of the scans around it; the same from launch to launch; one refusal per error the header lists; and `--ends` end
to end on the planted-end detection set."""
import ctypes as C
import os

import numpy as np
import pytest

import ends_cases as ec
import ends_oracle as orc
import tract_cases
from topsicle_amd import allsteps, hiplib, variants
from topsicle_amd import main as cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    with hiplib.HipScanner(0) as s:
        yield s


def _sketch(sc, slot, c):
    sc.upload(slot, *hiplib.pack_reads(list(c.reads)))
    return sc.end_sketch(slot, c.unit, c.tails, c.begin, c.end, c.k, c.buckets)


def test_sketch_before_any_table_and_every_case(sc):
    """The first thing this context does is a sketch: no tps_set_patterns has been called.  Then every case."""
    assert getattr(sc, "patterns", None) in (None, [])
    for c in ec.cases():
        got = _sketch(sc, 0, c)
        assert got[0].shape == (len(c.reads), c.buckets) and got[1].shape == (len(c.reads),)
        ec.assert_equal(got, c.name)


@pytest.mark.parametrize("name", ec.LINK_IDS)
def test_links_equal_oracle(sc, name):
    s, mm, ml = ec.link_sets()[name]
    ec.assert_links_equal(sc.sketch_links(s, mm, ml), ec.expected_links(name), name)


@pytest.fixture(scope="module")
def ragged():
    """60 reads of log-normal length with N, windows of 2000 at 100 (some past the read, some reads shorter than 100), both tails."""
    reads = list(tract_cases.ragged().reads[:60])
    n = len(reads)
    tails = [i & 1 for i in range(n)]
    begin, end = [100] * n, [2100] * n
    return reads, tails, begin, end, orc.end_sketch(reads, "CCCTAA", tails, begin, end)


def test_sketch_between_two_scans_changes_nothing(sc, ragged):
    reads, tails, begin, end, want = ragged
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
    got = sc.end_sketch(4, "CCCTAA", tails, begin, end)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (want[1] > 0).sum() > 30
    again = sc.results(4), sc.window_sums(4), sc.window_raw(4), sc.batch_trc_counts(4)           # as the scan left them
    second = scan()
    assert first[0]["pass"].sum() > 3
    for other in (again, second):
        assert np.array_equal(first[0], other[0])
        for a, b in zip(first[1] + first[2] + first[3], other[1] + other[2] + other[3]):
            assert np.array_equal(a, b)


def test_repeated_launches_give_identical_outputs(sc, ragged):
    reads, tails, begin, end, want = ragged
    sc.upload(5, *hiplib.pack_reads(reads))
    first = sc.end_sketch(5, "CCCTAA", tails, begin, end)
    for _ in range(3):
        again = sc.end_sketch(5, "CCCTAA", tails, begin, end)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    assert np.array_equal(first[0], want[0])
    s = ec.planted_sketches(400, 12)
    first = sc.sketch_links(s, 6, 16)
    for _ in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(first, sc.sketch_links(s, 6, 16)))


def test_links_on_1500_sketches_with_planted_groups(sc):
    """1500 random sketches, 30 planted groups of 10: the library's links equal the oracle's, row for row; some rows are cut."""
    s = ec.planted_sketches(1500, 30)
    for mm, ml in ((6, 64), (12, 4)):
        want = orc.sketch_links(s, mm, ml)
        ec.assert_links_equal(sc.sketch_links(s, mm, ml), want, f"planted mm{mm} ml{ml}")
    assert want[0].sum() > 300 and (want[0] > 4).any() and (want[0][300:] == 0).all()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw_sketch(sc, slot=3, code=None, m=6, k=12, buckets=256, tails=(0,), begin=(0,), end=(100,), lens=None):
    t, b, e = np.array(tails, np.uint8), np.array(begin, np.int32), np.array(end, np.int32)
    sk, kp = np.zeros(1024, np.uint32), np.zeros(4, np.uint32)
    nl, sl, kl = lens if lens is not None else (1, buckets, 1)
    return sc.lib.tps_batch_end_sketch(sc._h, slot, C.c_uint64(code), m, k, buckets, _p(t), _p(b), _p(e), nl, _p(sk), sl, _p(kp), kl)


@pytest.mark.parametrize("kw, code", ec.SKETCH_REFUSALS + [(dict(slot=9), "rc=-6")])
def test_sketch_refusals(sc, kw, code):
    """TPS_E_ARG = -3, TPS_E_CAPACITY = -5, TPS_E_STATE = -6 (a slot nothing was uploaded to); the call with that one argument
    corrected succeeds."""
    sc.upload(3, *hiplib.pack_reads(["ACGT" * 30]))
    good = dict(code=variants.unit_code("CCCTAA")[0])
    a = dict(good)
    a.update(kw)
    assert _raw_sketch(sc, **a) == int(code[3:])
    assert _raw_sketch(sc, **good) == 0 and _raw_sketch(sc, **dict(good, end=(16384,))) == 0


@pytest.mark.parametrize("kw, code", ec.LINK_REFUSALS)
def test_link_refusals(sc, kw, code):
    s = np.arange(128, dtype=np.uint32).reshape(2, 64)
    dg, ln, mt = np.zeros(2, np.int32), np.zeros(2 * 256, np.int32), np.zeros(2 * 256, np.int32)

    def call(min_match=6, max_links=4, buckets=None, lens=None, n=None):
        n = 2 if n is None else n
        b = 64 if buckets is None else buckets
        sl, dl, ll, tl = lens if lens is not None else (n * b, n, n * max_links, n * max_links)
        return sc.lib.tps_sketch_links(sc._h, _p(s), n, b, sl, min_match, max_links, _p(dg), dl, _p(ln), ll, _p(mt), tl)
    assert call(**kw) == int(code[3:])
    assert call() == 0


def _cli(argv):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args)


def test_cli_end_to_end_on_the_detection_set(tmp_path):
    """The 92 reads of the detection set through the CLI on the GPU, one pass and two: the same files, what the planted set asks
    for, telolengths_all.csv as without the flag."""
    ident = "CCCTAA_ONT"
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), ec.detection_reads(ident)[0])
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--gpus", "1"]
    _cli(common + ["-o", str(tmp_path / "plain")])
    _cli(common + ["-o", str(tmp_path / "one"), "--ends", "--twopass", "off"])
    _cli(common + ["-o", str(tmp_path / "two"), "--ends", "--twopass", "on"])
    read = lambda p: open(p, "rb").read()      # noqa: E731
    assert not os.path.exists(tmp_path / "plain" / "end_reads_4.csv")
    assert read(tmp_path / "plain" / "telolengths_all.csv") == read(tmp_path / "one" / "telolengths_all.csv") == read(tmp_path / "two" / "telolengths_all.csv")
    for f in ("end_reads_4.csv", "ends_4.csv"):
        assert read(tmp_path / "one" / f) == read(tmp_path / "two" / f)
    assert ec.check_cli_outputs(str(tmp_path / "one"), ident) >= 0.9 * ec.N_ENDS * ec.PER_END
    assert "end groups against CCCTAA" in open(tmp_path / "one" / "topsicle_run.log").read()
