"""The adapter search on the GPU (tps_batch_adapter_find; HipScanner.adapter_find), through the C ABI: bit for bit the plain dynamic
programme on the cases the emulation is checked on (tests/adapter_cases.py) and on the planted sets of the detection claim; the same rows
from a BAM-packed batch; independent of the pattern table and of the scans around it; the same from launch to launch and under two
fill bytes of the `poison` debug option; one refusal per error the header lists; and `--adapters` end to end on a planted set."""
import ctypes as C
import os

import numpy as np
import pytest

import adapter_cases as ac
import bam_tools as bt
import tract_cases
from topsicle_amd import allsteps, hiplib, seqio
from topsicle_amd import main as cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    with hiplib.HipScanner(0) as s:
        yield s


def test_before_any_table_and_every_case(sc):
    """The first thing this context does is an adapter search: no tps_set_patterns has been called.  Then every case."""
    assert getattr(sc, "patterns", None) in (None, [])
    for c in ac.cases():
        sc.upload(0, *hiplib.pack_reads(list(c.reads)))
        ac.assert_equal(sc.adapter_find(0, c.patterns, c.tails, c.begin, c.end), c.name)


def _nib4_batch(reads):
    """(nib, src, desc, n_words) of a BAM-packed batch that holds `reads`: every second one as a reverse-strand record."""
    nib, src = [], []
    off = 0
    for i, s in enumerate(reads):
        rev = bool(i & 1)
        stored = bt.revcomp(s.upper()) if rev else s.upper()
        codes = [bt.CODE[c] for c in stored] + ([0] if len(stored) & 1 else [])
        b = bytes((codes[j] << 4) | codes[j + 1] for j in range(0, len(codes), 2))
        pad = ((len(b) + 15) // 16) * 16
        nib.append(b + bytes(pad - len(b)))
        src.append((off, hiplib.NIB_REVERSE if rev else 0, 0))
        off += pad
    nib = np.frombuffer(b"".join(nib), np.uint8).copy()
    _seq2, _inv, desc = seqio.pack_reads_host(*hiplib.pack_reads([s.upper() for s in reads]))
    return nib, np.array(src, hiplib.NIB_SRC_DTYPE), desc.copy(), len(_seq2)


@pytest.mark.parametrize("name", ["letters", "regions_edges", "lengths"])
def test_bam_packed_batch_gives_the_same_rows(sc, name):
    c = ac.case(name)
    nib, src, desc, nw = _nib4_batch(list(c.reads))
    sc.upload_nib4(2, nib, src, desc, nw)
    ac.assert_equal(sc.adapter_find(2, c.patterns, c.tails, c.begin, c.end), name)


@pytest.mark.parametrize("ident", list(ac.SETS))
def test_detection_sets_equal_the_oracle(sc, ident):
    """The GPU's rows are the oracle's, on which tests/test_adapter.py holds the detection claim; the claim is asserted on them again."""
    pats, reads, tails, _planted, _ends = ac.detection_set(ident)
    n = len(reads)
    sc.upload(1, *hiplib.pack_reads(list(reads)))
    dist, end = sc.adapter_find(1, list(pats), tails, [0] * n, [ac.DETECT_SEARCH] * n)
    want = ac.detection_expected(ident)
    assert np.array_equal(dist, want[0]) and np.array_equal(end, want[1])
    ac.check_detection(dist, end, ident)


@pytest.fixture(scope="module")
def ragged():
    """60 reads of log-normal length with N, both tails, 64 patterns of mixed lengths cut out of the reads themselves."""
    reads = list(tract_cases.ragged().reads[:60])
    rng = np.random.default_rng(3)
    pats = []
    for j in range(64):
        src = reads[int(rng.integers(0, 60))].upper()
        m = int(rng.integers(12, 65))
        at = int(rng.integers(0, max(1, min(len(src), 300) - m)))
        p = "".join(ch if ch in "ACGT" else "A" for ch in src[at:at + m])
        pats.append(p + ac.rand(rng, m - len(p)))
    tails = [i & 1 for i in range(60)]
    return reads, pats, tails, [i % 23 for i in range(60)], [i % 23 + 300 + 11 * i for i in range(60)]


def test_call_between_two_scans_changes_nothing(sc, ragged):
    reads, pats, tails, begin, end = ragged
    sc.set_patterns(allsteps.patterns_to_search(telopattern="CCCTAA", cut_length=4))
    sc.upload(4, *hiplib.pack_reads(reads))
    prm = hiplib.make_params(min_len=500, min_count=20, window=100, slide=6, trimfirst=100, maxlen=20000,
                             flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS | hiplib.F_STORE_RAW)

    def scan():
        sc.scan(4, prm)
        sc.sync()
        return sc.results(4), sc.window_sums(4), sc.window_raw(4), sc.batch_trc_counts(4)
    first = scan()
    got = sc.adapter_find(4, pats, tails, begin, end)
    assert (got[0].min(axis=1) <= 6).sum() > 30                          # (the patterns come from the reads: many are found)
    again = sc.results(4), sc.window_sums(4), sc.window_raw(4), sc.batch_trc_counts(4)           # as the scan left them
    second = scan()
    assert first[0]["pass"].sum() > 3
    for other in (again, second):
        assert np.array_equal(first[0], other[0])
        for a, b in zip(first[1] + first[2] + first[3], other[1] + other[2] + other[3]):
            assert np.array_equal(a, b)
    assert all(np.array_equal(a, b) for a, b in zip(got, sc.adapter_find(4, pats, tails, begin, end)))


def test_repeated_launches_and_two_poison_bytes_give_identical_outputs(sc, ragged):
    reads, pats, tails, begin, end = ragged
    sc.upload(5, *hiplib.pack_reads(reads))
    first = sc.adapter_find(5, pats, tails, begin, end)
    for _ in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(first, sc.adapter_find(5, pats, tails, begin, end)))
    try:
        for fill in (0x5A, 0xA5):
            sc.debug_option("poison", fill)
            assert all(np.array_equal(a, b) for a, b in zip(first, sc.adapter_find(5, pats, tails, begin, end))), fill
            # fewer patterns and fewer reads in buffers that held more: what is handed out is what this call wrote
            sc.upload(6, *hiplib.pack_reads(reads[:7]))
            few = sc.adapter_find(6, pats[:3], tails[:7], begin[:7], end[:7])
            assert np.array_equal(few[0], first[0][:7, :3]) and np.array_equal(few[1], first[1][:7, :3]), fill
    finally:
        sc.debug_option("poison", 0)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw(sc, slot=3, n_pat=1, pat_len=12, code=(0, 0), tail=0, begin=0, end=100, n_reads=1, hits_len=None):
    pats = np.array([code] * max(n_pat, 1), np.uint64)
    lens = np.array([pat_len] * max(n_pat, 1), np.int32)
    t, b, e = np.array([tail], np.uint8), np.array([begin], np.int32), np.array([end], np.int32)
    hits = np.zeros(2 * 64 + 2, np.uint16)
    return sc.lib.tps_batch_adapter_find(sc._h, slot, _p(pats), _p(lens), n_pat, _p(t), _p(b), _p(e), n_reads, _p(hits),
                                         2 * max(n_pat, 0) if hits_len is None else hits_len)


@pytest.mark.parametrize("kw, code", ac.REFUSALS + [(dict(slot=9), "rc=-6")])
def test_refusals(sc, kw, code):
    """TPS_E_ARG = -3, TPS_E_CAPACITY = -5, TPS_E_STATE = -6 (a slot nothing was uploaded to); the call with that one argument
    corrected succeeds."""
    sc.upload(3, *hiplib.pack_reads(["ACGT" * 30]))
    assert _raw(sc, **kw) == int(code[3:])
    assert _raw(sc) == 0 and _raw(sc, n_pat=64) == 0 and _raw(sc, end=1024) == 0 and _raw(sc, pat_len=64, code=((1 << 64) - 1, (1 << 64) - 1)) == 0


def _cli(argv):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args)


def test_cli_end_to_end_on_a_planted_set(tmp_path):
    """48 reads of a planted set through the CLI on the GPU, one pass and two: the same files, what the planted set asks for, every
    other file as without the flag."""
    d, fa = ac.write_cli_inputs(tmp_path)
    common = ["-i", d, "--pattern", "CCCTAA", "--minSeqLength", "1000", "--cutoff", "0.4", "--gpus", "1"]
    _cli(common + ["-o", str(tmp_path / "plain")])
    _cli(common + ["-o", str(tmp_path / "one"), "--adapters", fa, "--twopass", "off"])
    _cli(common + ["-o", str(tmp_path / "two"), "--adapters", fa, "--twopass", "on"])
    read = lambda p: open(p, "rb").read()      # noqa: E731
    assert not os.path.exists(tmp_path / "plain" / "adapters_4.csv")
    others = sorted(f for f in os.listdir(tmp_path / "plain") if f != "topsicle_run.log")
    assert "telolengths_all.csv" in others
    for f in others:
        assert read(tmp_path / "plain" / f) == read(tmp_path / "one" / f) == read(tmp_path / "two" / f), f
    for f in ("adapters_4.csv", "adapter_summary_4.csv"):
        assert read(tmp_path / "one" / f) == read(tmp_path / "two" / f)
    n_rows, named = ac.check_cli_outputs(str(tmp_path / "one"))
    assert n_rows >= 30 and named >= 20
    assert "adapters: 12 sequences" in open(tmp_path / "one" / "topsicle_run.log").read()
