"""Named ends on the GPU (tps_window_place; HipScanner.place_windows), through the C ABI: equal to the plain restatement of the rule on
the cases the emulation is checked on (tests/place_cases.py); independent of the pattern table and of the scans around it; the same
from launch to launch and under two fill bytes of the `poison` debug option; one refusal per error the header lists; and
`--ends --endref` end to end on the planted-end detection set."""
import ctypes as C
import os

import numpy as np
import pytest

import anchor_cases as ac
import ends_cases as ec
import place_cases as pc
import tract_cases
from topsicle_amd import allsteps, hiplib
from topsicle_amd import main as cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    with hiplib.HipScanner(0) as s:
        yield s


def test_before_any_table_and_every_case(sc):
    """The first thing this context does is a placement: no tps_set_patterns has been called, no batch uploaded.  Then every case."""
    assert getattr(sc, "patterns", None) in (None, [])
    pc.assert_equal(pc.run_case(sc.place_windows, "ties"), pc.expected("ties"), "ties")
    for name in pc.CASE_IDS:
        pc.assert_equal(pc.run_case(sc.place_windows, name), pc.expected(name), name)


@pytest.fixture(scope="module")
def planted():
    """The 92 windows of a planted set (the oracle's rows) and the windows of six of its reads, one per planted end, as the reference."""
    rows = ac.detection_rows("CCCTAA_ONT")
    truth = ec.detection_reads("CCCTAA_ONT")[1]
    first = [truth.index(e) for e in range(1, ec.N_ENDS + 1)]
    return rows["codes"], rows["keep"], rows["length"], rows["codes"][first], rows["keep"][first], rows["length"][first], ec.SPAN, ec.K


def test_call_between_two_scans_changes_nothing(sc, planted):
    reads = list(tract_cases.ragged().reads[:60])
    sc.set_patterns(allsteps.patterns_to_search(telopattern="CCCTAA", cut_length=4))
    sc.upload(4, *hiplib.pack_reads(reads))
    prm = hiplib.make_params(min_len=500, min_count=20, window=100, slide=6, trimfirst=100, maxlen=20000,
                             flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS | hiplib.F_STORE_RAW)

    def scan():
        sc.scan(4, prm)
        sc.sync()
        return sc.results(4), sc.window_sums(4), sc.window_raw(4), sc.batch_trc_counts(4)
    first = scan()
    got = sc.place_windows(*planted)
    truth = np.array(ec.detection_reads("CCCTAA_ONT")[1])
    assert (got[0][truth > 0] == truth[truth > 0] - 1).all() and (got[5][truth > 0] > 100).all() and (got[5][truth == 0] < 20).all()
    again = sc.results(4), sc.window_sums(4), sc.window_raw(4), sc.batch_trc_counts(4)           # as the scan left them
    second = scan()
    assert first[0]["pass"].sum() > 3
    for other in (again, second):
        assert np.array_equal(first[0], other[0])
        for a, b in zip(first[1] + first[2] + first[3], other[1] + other[2] + other[3]):
            assert np.array_equal(a, b)


def test_repeated_launches_and_two_fill_bytes_give_identical_outputs(sc, planted):
    first = sc.place_windows(*planted)
    for _ in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(first, sc.place_windows(*planted)))
    try:
        for fill in (0x5A, 0xA5):
            sc.debug_option("poison", fill)
            assert all(np.array_equal(a, b) for a, b in zip(first, sc.place_windows(*planted))), hex(fill)
            name = "many_refs"                     # (another shape in the same buffers: what the call before left behind does not show)
            pc.assert_equal(pc.run_case(sc.place_windows, name), pc.expected(name), name)
    finally:
        sc.debug_option("poison", 0)
    assert all(np.array_equal(a, b) for a, b in zip(first, sc.place_windows(*planted)))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("kw, code", pc.REFUSALS)
def test_refusals(sc, kw, code):
    """TPS_E_ARG = -3, TPS_E_CAPACITY = -5; the call with that one argument corrected succeeds."""
    r = pc.REFUSAL_ROWS
    out = [np.full(4, 77, np.int32) for _ in range(7)]

    def call(length, ref_length, span, k, max_occ, lens):
        ln, rl = np.array(length, np.int32), np.array(ref_length, np.int32)
        cl, kl, n, rcl, rkl, n_ref, ol = pc.GOOD_LENS if lens is None else lens
        return sc.lib.tps_window_place(sc._h, _p(r["codes"]), cl, _p(r["keep"]), kl, _p(ln), n, _p(r["ref_codes"]), rcl, _p(r["ref_keep"]), rkl, _p(rl), n_ref,
                                       span, k, max_occ, *[_p(o) for o in out], ol)
    assert call(**dict(pc.GOOD, **kw)) == int(code[3:])
    assert all((o == 77).all() for o in out)                                                # a refused call writes nothing
    assert call(**pc.GOOD) == 0
    assert [o[:2].tolist() for o in out] == [[-1, -1], [0, 0], [-1, -1], [0, 0], [0, 0], [0, 0], [0, 0]] and all((o[2:] == 77).all() for o in out)


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
    pc.write_reference(str(tmp_path / "ref.fasta"), ident)
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--gpus", "1", "--ends"]
    _cli(common + ["-o", str(tmp_path / "ends")])
    _cli(common + ["-o", str(tmp_path / "one"), "--endref", str(tmp_path / "ref.fasta"), "--twopass", "off"])
    _cli(common + ["-o", str(tmp_path / "two"), "--endref", str(tmp_path / "ref.fasta"), "--twopass", "on"])
    read = lambda p: open(p, "rb").read()      # noqa: E731
    new = ("ref_ends_4.csv", "named_reads_4.csv", "named_ends_4.csv")
    others = sorted(f for f in os.listdir(tmp_path / "ends") if f != "topsicle_run.log")
    assert "telolengths_all.csv" in others and "end_reads_4.csv" in others and "ends_4.csv" in others
    for run in ("one", "two"):
        assert sorted(f for f in os.listdir(tmp_path / run) if f != "topsicle_run.log" and f not in new) == others
        for f in others:
            assert read(tmp_path / "ends" / f) == read(tmp_path / run / f), f
    for f in new:
        assert not os.path.exists(tmp_path / "ends" / f) and read(tmp_path / "one" / f) == read(tmp_path / "two" / f)
    errors, n_named = pc.check_cli_outputs(str(tmp_path / "one"), ident)
    p95, worst = ac.BOUNDS["ONT"]
    print(f"--ends --endref on {ident}: {n_named} reads named; error of ref_length median / p95 / max {np.median(errors):.0f} / {np.percentile(errors, 95):.0f} / {errors[-1]}")
    assert np.percentile(errors, 95) <= p95 and errors[-1] <= worst
    assert "named ends: 6 of 6 reference pieces" in open(tmp_path / "one" / "topsicle_run.log").read()
