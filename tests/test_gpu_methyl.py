"""Base modifications against the boundary on the GPU (tps_batch_mod_profile; HipScanner.mod_profile), through the C ABI: bit for bit
the plain rule on the cases the emulation is checked on (tests/methyl_cases.py); a slot other than 0 and a subset of the reads;
independent of the pattern table and of the scans around it; the same from launch to launch, under two fills of the caller's arrays
and two fill bytes of the `poison` debug option; every refusal with the emulation's code and words; and `--methyl` end to end on a
BAM file, its files equal to the emulation's."""
import ctypes as C
import os

import numpy as np
import pytest

import bam_tools
import methyl_cases as mc
from test_methyl import _One, check_methyl_run, emu_refusal
from topsicle_amd import allsteps, hiplib
from topsicle_amd import main as cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    with hiplib.HipScanner(0) as s:
        yield s


def _run(sc, slot, c, idx=None):
    pick = (lambda x: list(x)) if idx is None else (lambda x: [x[i] for i in idx])
    sc.upload(slot, *hiplib.pack_reads(pick(c.reads)))
    return sc.mod_profile(slot, pick(c.tails), pick(c.begin), pick(c.end), pick(c.origin), *c.lists(idx), **c.kw())


@pytest.mark.parametrize("name", mc.names())
def test_every_case_equals_the_oracle(sc, name):
    """(the first case is the first thing this context does: no tps_set_patterns has been called)"""
    mc.assert_equal(_run(sc, 0, mc.case(name)), name)


def test_another_slot_and_a_subset_of_the_reads(sc):
    c = mc.case("mixed")
    idx = [i for i in range(len(c.reads)) if i % 3 != 1]          # what the second pass of the two-pass route holds: some of the reads
    mc.assert_equal(_run(sc, 5, c, idx), "mixed", idx)
    mc.assert_equal(_run(sc, 7, mc.case("regions"), [4, 2, 9]), "regions", [4, 2, 9])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw(sc, slot, c, rows, bins, lists=None, n_reads=None, rows_len=None, bins_len=None, **kw):
    """The C call itself on the reads resident in `slot`, rows and bins into the arrays as they stand."""
    arr = {k: np.ascontiguousarray(kw.pop(k, getattr(c, k)), dt) for k, dt in (("tails", np.uint8), ("begin", np.int32), ("end", np.int32), ("origin", np.int32))}
    off, delta, prob = lists if lists is not None else c.lists()
    off = np.ascontiguousarray(kw.pop("mod_off", off), np.int64)
    w = dict(c.kw(), **kw)
    return sc.lib.tps_batch_mod_profile(sc._h, slot, _p(arr["tails"]), _p(arr["begin"]), _p(arr["end"]), _p(arr["origin"]),
                                        len(arr["tails"]) if n_reads is None else n_reads, _p(off), _p(delta), _p(prob), len(delta), w["w"], w["nb0"], w["nb1"],
                                        w["hi"], w["lo"], _p(rows), len(rows) if rows_len is None else rows_len, _p(bins), bins.size if bins_len is None else bins_len)


def test_repeated_launches_two_fills_and_two_poison_bytes_give_identical_outputs(sc):
    c = mc.case("mixed")
    want_rows, want_bins = mc.expected("mixed")
    first = _run(sc, 2, c)
    mc.assert_equal(first, "mixed")
    for _ in range(2):
        mc.assert_equal(sc.mod_profile(2, c.tails, c.begin, c.end, c.origin, *c.lists(), **c.kw()), "mixed")
    for fill in (0x00, 0xFF):                      # every row and record is written whole: what the caller's arrays held does not show
        rows = np.frombuffer(bytes([fill]) * (32 * len(want_rows)), hiplib.MOD_ROW_DTYPE).copy()
        bins = np.frombuffer(bytes([fill]) * (12 * want_bins.size), hiplib.MOD_BIN_DTYPE).copy().reshape(want_bins.shape)
        assert _raw(sc, 2, c, rows, bins) == 0
        mc.assert_equal((rows, bins), "mixed")
    try:
        for fill in (0x5A, 0xA5):
            sc.debug_option("poison", fill)
            mc.assert_equal(sc.mod_profile(2, c.tails, c.begin, c.end, c.origin, *c.lists(), **c.kw()), "mixed")
            # fewer and shorter reads in buffers that held more: what is handed out is what this call wrote
            mc.assert_equal(_run(sc, 6, mc.case("no_c_last_c")), "no_c_last_c")
    finally:
        sc.debug_option("poison", 0)


def test_call_between_two_scans_changes_nothing(sc):
    c = mc.case("mixed")
    sc.set_patterns(allsteps.patterns_to_search(telopattern="CCCTAA", cut_length=4))
    sc.upload(4, *hiplib.pack_reads(list(c.reads)))
    prm = hiplib.make_params(min_len=500, min_count=0, window=100, slide=6, trimfirst=100, maxlen=20000,
                             flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS | hiplib.F_STORE_RAW)

    def state():
        return sc.results(4), sc.window_sums(4), sc.window_raw(4), sc.batch_trc_counts(4)

    def scan():
        sc.scan(4, prm)
        sc.sync()
        return state()
    first = scan()
    mc.assert_equal(sc.mod_profile(4, c.tails, c.begin, c.end, c.origin, *c.lists(), **c.kw()), "mixed")
    again = state()                                # results (the tails among them), sums and rows as the scan left them
    second = scan()
    assert first[0]["pass"].sum() > 3
    for other in (again, second):
        assert np.array_equal(first[0], other[0])
        for a, b in zip(first[1] + first[2] + first[3], other[1] + other[2] + other[3]):
            assert np.array_equal(a, b)


class _OneCase(_One):
    @staticmethod
    def kw():
        return dict(w=500, nb0=2, nb1=8, hi=205, lo=50)


_ONE_LISTS = (np.array(_One.mod_off, np.int64), np.array(_One.delta, np.uint32), np.array(_One.prob, np.uint8))


@pytest.mark.parametrize("kw, code, text", mc.REFUSALS)
def test_refusals_hold_the_emulations_code_and_words(sc, kw, code, text):
    sc.upload(3, *hiplib.pack_reads(_One.reads))
    rows, bins = np.zeros(2, hiplib.MOD_ROW_DTYPE), np.zeros(80, hiplib.MOD_BIN_DTYPE)
    nb = max(0, kw.get("nb0", 2) + kw.get("nb1", 8))           # (the bins the call's own nb0 + nb1 ask for, unless bins_len is what is wrong)
    assert _raw(sc, 3, _OneCase, rows[:1], bins[:nb], _ONE_LISTS, **kw) == int(code[3:])
    msg = sc.lib.tps_last_error().decode()
    assert text in msg and msg == emu_refusal(_One.reads, kw).split(": ", 1)[1]
    assert _raw(sc, 3, _OneCase, rows[:1], bins[:10], _ONE_LISTS) == 0 and rows["in_region"][0] == 2 and bins["called"][:3].tolist() == [0, 2, 0]
    assert _raw(sc, 3, _OneCase, rows[:1], bins[:1], _ONE_LISTS, w=4096, nb0=0, nb1=1, hi=255, lo=0, origin=[0], end=[1 << 30]) == 0


def test_empty_slot_region_cap_and_empty_batch(sc):
    rows, bins = np.zeros(2, hiplib.MOD_ROW_DTYPE), np.zeros(10, hiplib.MOD_BIN_DTYPE)
    assert _raw(sc, 9, _OneCase, rows[:1], bins, _ONE_LISTS) == -6                           # TPS_E_STATE: nothing uploaded there
    kw, code, text = mc.LONG_REFUSAL
    reads = ["ACGT" * 4100] * 2
    sc.upload(3, *hiplib.pack_reads(reads))
    two = dict(tails=[0, 1], origin=[0, 0], mod_off=[0, 1, 2], w=4096, nb0=0, nb1=5)
    assert _raw(sc, 3, _OneCase, rows, bins, _ONE_LISTS, **two, **kw) == int(code[3:])
    msg = sc.lib.tps_last_error().decode()
    assert text in msg and msg == emu_refusal(reads, dict(two, **kw)).split(": ", 1)[1]
    assert _raw(sc, 3, _OneCase, rows, bins, _ONE_LISTS, **two, begin=[0, 16], end=[16384, 1 << 30]) == 0      # 16 384 each: end is clamped first
    assert rows["cpg"].tolist() == [4096, 4096] and bins["cpg"].tolist() == [1024] * 4 + [0] + [1020, 1024, 1024, 1024, 4]
    sc.upload(3, *hiplib.pack_reads([]))
    none = np.zeros(0, np.int32)
    empty = (np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint8))
    assert _raw(sc, 3, _OneCase, np.zeros(0, hiplib.MOD_ROW_DTYPE), np.zeros(0, hiplib.MOD_BIN_DTYPE), empty, tails=none, begin=none, end=none, origin=none) == 0


def _cli(argv, engines=None):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


def test_cli_end_to_end_equals_the_emulations_files(tmp_path):
    """The BAM fixture once on the device: its files are the oracle's rows and, byte for byte, those of the run on the emulation
    engines; every other file is as without the flag."""
    import emu_adapter_driver
    import emu_anchor_driver
    import emu_driver
    import emu_ends_driver
    import emu_follow_wide_driver
    import emu_methyl_driver
    import emu_motif_driver
    import emu_refine_driver
    import emu_variant_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver, emu_variant_driver, emu_ends_driver, emu_anchor_driver, emu_adapter_driver,
              emu_refine_driver, emu_methyl_driver):
        d.build()
    from emu_methyl_engine import EmuMethylEngine
    reads, truth = mc.cli_bam_reads()
    d = tmp_path / "in"
    d.mkdir()
    bam_tools.write_bam(str(d / "reads.bam"), reads)
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--gpus", "1"]
    _cli(common + ["-o", str(tmp_path / "plain")])
    _cli(common + ["-o", str(tmp_path / "gpu"), "--methyl", "--ends", "--endminreads", "1", "--endminkmers", "10"])
    _cli(common + ["-o", str(tmp_path / "emu"), "--methyl", "--ends", "--endminreads", "1", "--endminkmers", "10"], [EmuMethylEngine(), EmuMethylEngine()])
    read = lambda p: open(p, "rb").read()      # noqa: E731
    assert not os.path.exists(tmp_path / "plain" / "methyl_4.csv")
    others = sorted(f for f in os.listdir(tmp_path / "plain") if f != "topsicle_run.log")
    assert "telolengths_all.csv" in others
    for f in others:
        assert read(tmp_path / "plain" / f) == read(tmp_path / "gpu" / f), f
    for f in ("methyl_4.csv", "methyl_profile_4.csv", "methyl_ends_4.csv", "end_reads_4.csv", "ends_4.csv"):
        assert read(tmp_path / "gpu" / f) == read(tmp_path / "emu" / f), f
    check_methyl_run(tmp_path / "gpu", reads, truth)
    assert "methylation: " in open(tmp_path / "gpu" / "topsicle_run.log").read()
