"""Anchored lengths on the GPU (tps_batch_end_window, tps_window_offsets; HipScanner.end_window, HipScanner.anchor_offsets), through
the C ABI: equal to the plain restatement of the rules on the cases the emulation is checked on (tests/anchor_cases.py); independent
of the pattern table and of the scans around it; the same from launch to launch; one refusal per error the header lists; and
`--ends --anchor` end to end on the planted-end detection set."""
import ctypes as C
import os

import numpy as np
import pytest

import anchor_cases as ac
import anchor_oracle as orc
import ends_cases as ec
import tract_cases
from topsicle_amd import allsteps, hiplib, variants
from topsicle_amd import main as cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    with hiplib.HipScanner(0) as s:
        yield s


def test_both_before_any_table_and_every_case(sc):
    """The first thing this context does is an offsets call, the second a window extraction: no tps_set_patterns has been called.  Then
    every case: the extraction where the case has reads, the offsets over the oracle's rows and over the library's own."""
    assert getattr(sc, "patterns", None) in (None, [])
    c, want = ac.case("median"), ac.expected("median")
    ac.assert_offsets_equal(sc.anchor_offsets(want["codes"], want["keep"], want["length"], c.ref, c.span, c.k), "median")
    for c in ac.cases():
        want = ac.expected(c.name)
        codes, keep = want["codes"], want["keep"]
        if not c.by_hand:
            sc.upload(0, *hiplib.pack_reads(list(c.reads)))
            codes, keep = sc.end_window(0, c.unit, c.tails, c.begin, c.end, c.k, c.span)
            ac.assert_rows_equal((codes, keep), c.name)
        ac.assert_offsets_equal(sc.anchor_offsets(codes, keep, want["length"], c.ref, c.span, c.k), c.name)


@pytest.fixture(scope="module")
def ragged():
    """60 reads of log-normal length with N, windows of 2000 at 100 (some past the read, some reads shorter than 100), both tails; every
    row against row 7."""
    reads = list(tract_cases.ragged().reads[:60])
    n = len(reads)
    tails = [i & 1 for i in range(n)]
    begin, end = [100] * n, [2100] * n
    codes, keep, windows, keeps = orc.end_window(reads, "CCCTAA", tails, begin, end)
    return reads, tails, begin, end, (codes, keep), np.array([len(w) for w in windows], np.int32)


def test_window_between_two_scans_changes_nothing(sc, ragged):
    reads, tails, begin, end, want, _length = ragged
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
    got = sc.end_window(4, "CCCTAA", tails, begin, end)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (ac.popcount(want[1]) > 0).sum() > 30
    assert np.array_equal(ac.popcount(got[1]), sc.end_sketch(4, "CCCTAA", tails, begin, end)[1])          # popcount(keep) == kept
    again = sc.results(4), sc.window_sums(4), sc.window_raw(4), sc.batch_trc_counts(4)           # as the scan left them
    second = scan()
    assert first[0]["pass"].sum() > 3
    for other in (again, second):
        assert np.array_equal(first[0], other[0])
        for a, b in zip(first[1] + first[2] + first[3], other[1] + other[2] + other[3]):
            assert np.array_equal(a, b)


def test_repeated_launches_give_identical_outputs(sc, ragged):
    reads, tails, begin, end, want, length = ragged
    sc.upload(5, *hiplib.pack_reads(reads))
    first = sc.end_window(5, "CCCTAA", tails, begin, end)
    ref = [7] * len(reads)
    offs = sc.anchor_offsets(first[0], first[1], length, ref, 2000)
    for _ in range(3):
        again = sc.end_window(5, "CCCTAA", tails, begin, end)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
        assert all(np.array_equal(a, b) for a, b in zip(offs, sc.anchor_offsets(first[0], first[1], length, ref, 2000)))
    assert np.array_equal(first[0], want[0]) and np.array_equal(first[1], want[1])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw_window(sc, slot=3, code=None, m=6, k=12, span=100, tails=(0,), begin=(0,), end=(100,), lens=None):
    t, b, e = np.array(tails, np.uint8), np.array(begin, np.int32), np.array(end, np.int32)
    co, kp = np.zeros(1024, np.uint32), np.zeros(512, np.uint32)
    nl, cl, kl = lens if lens is not None else (1, (span + 15) // 16, (span + 31) // 32)
    return sc.lib.tps_batch_end_window(sc._h, slot, C.c_uint64(code), m, k, _p(t), _p(b), _p(e), nl, span, _p(co), cl, _p(kp), kl)


@pytest.mark.parametrize("kw, code", ac.WINDOW_REFUSALS + [(dict(slot=9), "rc=-6")])
def test_window_refusals(sc, kw, code):
    """TPS_E_ARG = -3, TPS_E_CAPACITY = -5, TPS_E_STATE = -6 (a slot nothing was uploaded to); the call with that one argument
    corrected succeeds."""
    sc.upload(3, *hiplib.pack_reads(["ACGT" * 30]))
    good = dict(code=variants.unit_code("CCCTAA")[0])
    a = dict(good)
    a.update(kw)
    assert _raw_window(sc, **a) == int(code[3:])
    assert _raw_window(sc, **good) == 0 and _raw_window(sc, **dict(good, span=4096, end=(4096,))) == 0


@pytest.mark.parametrize("kw, code", ac.OFFSET_REFUSALS)
def test_offset_refusals(sc, kw, code):
    codes, keep = np.zeros(2 * 7, np.uint32), np.zeros(2 * 4, np.uint32)
    out = [np.zeros(4, np.int32) for _ in range(3)]

    def call(length=(100, 5), ref=(1, -7), span=100, k=12, n=None, out_len=None):
        n = 2 if n is None else n
        ln, rf = np.array(length, np.int32), np.array(ref, np.int32)
        return sc.lib.tps_window_offsets(sc._h, _p(codes), _p(keep), _p(ln), _p(rf), n, span, k, _p(out[0]), _p(out[1]), _p(out[2]), n if out_len is None else out_len)
    assert call(**kw) == int(code[3:])
    assert call() == 0


def _cli(argv):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args)


def test_cli_end_to_end_on_the_detection_set(tmp_path):
    """The 92 reads of the detection set through the CLI on the GPU, one pass and two: the same files, what the planted set asks
    for, every other file as without the flag."""
    ident = "CCCTAA_ONT"
    d = tmp_path / "in"
    d.mkdir()
    ec.write_fasta(str(d / "reads.fasta"), ec.detection_reads(ident)[0])
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--gpus", "1", "--ends"]
    _cli(common + ["-o", str(tmp_path / "ends")])
    _cli(common + ["-o", str(tmp_path / "one"), "--anchor", "--twopass", "off"])
    _cli(common + ["-o", str(tmp_path / "two"), "--anchor", "--twopass", "on"])
    read = lambda p: open(p, "rb").read()      # noqa: E731
    assert not os.path.exists(tmp_path / "ends" / "anchored_reads_4.csv")
    for f in ("telolengths_all.csv", "end_reads_4.csv", "ends_4.csv"):
        assert read(tmp_path / "ends" / f) == read(tmp_path / "one" / f) == read(tmp_path / "two" / f)
    for f in ("anchored_reads_4.csv", "anchored_ends_4.csv"):
        assert read(tmp_path / "one" / f) == read(tmp_path / "two" / f)
    anchored_err, _called_err, n_anchored = ac.check_cli_outputs(str(tmp_path / "one"), ident)
    p95, worst = ac.BOUNDS["ONT"]
    assert n_anchored >= 0.9 * ec.N_ENDS * ec.PER_END and np.percentile(anchored_err, 95) <= p95 and anchored_err[-1] <= worst
    assert "anchored lengths: " in open(tmp_path / "one" / "topsicle_run.log").read()
