"""The boundary at base resolution on the GPU (tps_batch_boundary_refine; HipScanner.boundary_refine), through the C ABI: bit for bit
the plain rule on the cases the emulation is checked on (tests/refine_cases.py); a slot other than 0 and a subset of the reads;
independent of the pattern table and of the scans around it; the same from launch to launch, under two fills of the caller's rows and
two fill bytes of the `poison` debug option; every refusal with the emulation's code and words; and `--refine` end to end, its files
equal to the emulation's."""
import ctypes as C
import os

import numpy as np
import pytest

import emu_refine_driver as emu
import refine_cases as rc
import variant_cases as vc
from topsicle_amd import allsteps, hiplib, variants
from topsicle_amd import main as cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    with hiplib.HipScanner(0) as s:
        yield s


def _run(sc, slot, c, idx=None):
    pick = (lambda x: list(x)) if idx is None else (lambda x: [x[i] for i in idx])
    sc.upload(slot, *hiplib.pack_reads(pick(c.reads)))
    return sc.boundary_refine(slot, c.unit, pick(c.tails), pick(c.begin), pick(c.end), pick(c.at), **c.kw())


@pytest.mark.parametrize("name", rc.names())
def test_every_case_equals_the_oracle(sc, name):
    """(the first case is the first thing this context does: no tps_set_patterns has been called)"""
    rc.assert_equal(_run(sc, 0, rc.case(name)), name)


def test_another_slot_and_a_subset_of_the_reads(sc):
    c = rc.case("ragged")
    want = rc.expected("ragged")
    idx = [i for i in range(len(c.reads)) if i % 3 != 1][:150]          # what the second pass of the two-pass route holds: some of the reads
    got = _run(sc, 5, c, idx)
    assert np.array_equal(got, want[idx])
    c = rc.case("runner")
    assert np.array_equal(_run(sc, 7, c, [4, 2, 9]), rc.expected("runner")[[4, 2, 9]])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw(sc, slot, c, out, n_reads=None, out_len=None, **kw):
    """The C call itself on the reads resident in `slot`, the rows into `out` as it stands."""
    code, m = kw.pop("unit") if isinstance(kw.get("unit"), tuple) else variants.unit_code(kw.pop("unit", c.unit))
    arr = {k: np.ascontiguousarray(kw.pop(k, getattr(c, k)), dt) for k, dt in (("tails", np.uint8), ("begin", np.int32), ("end", np.int32), ("at", np.int32))}
    w = dict(c.kw(), **kw)
    return sc.lib.tps_batch_boundary_refine(sc._h, slot, C.c_uint64(code), m, _p(arr["tails"]), _p(arr["begin"]), _p(arr["end"]), _p(arr["at"]),
                                            len(arr["tails"]) if n_reads is None else n_reads, w["hit"], w["miss"], w["sep"], _p(out),
                                            len(out) if out_len is None else out_len)


def test_repeated_launches_two_fills_and_two_poison_bytes_give_identical_rows(sc):
    c = rc.case("ragged")
    want = rc.expected("ragged")
    first = _run(sc, 2, c)
    assert np.array_equal(first, want)
    for _ in range(2):
        assert np.array_equal(first, sc.boundary_refine(2, c.unit, c.tails, c.begin, c.end, c.at, **c.kw()))
    for fill in (0x00, 0xFF):                      # every row is written whole: what the caller's array held does not show
        out = np.frombuffer(bytes([fill]) * (32 * len(want)), hiplib.REFINE_DTYPE).copy()
        assert _raw(sc, 2, c, out) == 0 and np.array_equal(out, want), fill
    try:
        for fill in (0x5A, 0xA5):
            sc.debug_option("poison", fill)
            assert np.array_equal(first, sc.boundary_refine(2, c.unit, c.tails, c.begin, c.end, c.at, **c.kw())), fill
            # fewer and shorter reads in buffers that held more: what is handed out is what this call wrote
            few = rc.case("at")
            assert np.array_equal(_run(sc, 6, few), rc.expected("at")), fill
    finally:
        sc.debug_option("poison", 0)


def test_call_between_two_scans_changes_nothing(sc):
    c = rc.case("ragged")
    sc.set_patterns(allsteps.patterns_to_search(telopattern="CCCTAA", cut_length=4))
    sc.upload(4, *hiplib.pack_reads(list(c.reads)))
    prm = hiplib.make_params(min_len=500, min_count=20, window=100, slide=6, trimfirst=100, maxlen=20000,
                             flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS | hiplib.F_STORE_RAW)

    def state():
        return sc.results(4), sc.window_sums(4), sc.window_raw(4), sc.batch_trc_counts(4)

    def scan():
        sc.scan(4, prm)
        sc.sync()
        return state()
    first = scan()
    got = sc.boundary_refine(4, c.unit, c.tails, c.begin, c.end, c.at, **c.kw())
    assert np.array_equal(got, rc.expected("ragged"))
    again = state()                                # results (the tails among them), sums and rows as the scan left them
    second = scan()
    assert first[0]["pass"].sum() > 3
    for other in (again, second):
        assert np.array_equal(first[0], other[0])
        for a, b in zip(first[1] + first[2] + first[3], other[1] + other[2] + other[3]):
            assert np.array_equal(a, b)


class _One:
    """The good call of the refusal tests: one read of 120 letters."""
    reads, unit, tails, begin, end, at = ["ACGT" * 30], "CCCTAA", [0], [0], [100], [50]

    @staticmethod
    def kw():
        return dict(hit=2, miss=1, sep=200)


def _emu_message(reads, kw):
    k = dict(kw)
    lens = (k.pop("n_reads", len(reads)), k.pop("out_len", len(reads)))
    args = {f: k.pop(f, getattr(_One, f)) for f in ("unit", "tails", "begin", "end", "at")}
    with pytest.raises(hiplib.TopsicleHipError) as e:
        emu.boundary_refine(reads, args["unit"], args["tails"], args["begin"], args["end"], args["at"], lens=lens, **dict(_One.kw(), **k))
    return str(e.value).split(": ", 1)[1]


@pytest.mark.parametrize("kw, code, text", rc.REFUSALS)
def test_refusals_hold_the_emulations_code_and_words(sc, kw, code, text):
    sc.upload(3, *hiplib.pack_reads(_One.reads))
    out = np.zeros(2, hiplib.REFINE_DTYPE)
    assert _raw(sc, 3, _One, out[:1], **kw) == int(code[3:])
    msg = sc.lib.tps_last_error().decode()
    assert text in msg and msg == _emu_message(_One.reads, kw)
    assert _raw(sc, 3, _One, out[:1]) == 0 and _raw(sc, 3, _One, out[:1], hit=16, miss=16, sep=65535, end=[1 << 30]) == 0


def test_empty_slot_region_cap_and_empty_batch(sc):
    out = np.zeros(2, hiplib.REFINE_DTYPE)
    assert _raw(sc, 9, _One, out[:1]) == -6                                                  # TPS_E_STATE: nothing uploaded there
    kw, code, text = rc.LONG_REFUSAL
    reads = ["ACGT" * 16400] * 2
    sc.upload(3, *hiplib.pack_reads(reads))
    two = dict(tails=[0, 1], at=[0, 0])
    assert _raw(sc, 3, _One, out, **two, **kw) == int(code[3:])
    msg = sc.lib.tps_last_error().decode()
    assert text in msg and msg == _emu_message(reads, dict(two, **kw))
    assert _raw(sc, 3, _One, out, **two, begin=[0, 64], end=[65536, 1 << 30]) == 0          # 65 536 each: end is clamped first
    assert out["pos"].tolist() == [0, 64] and (out["drop"] == 65536 - 5).all()
    sc.upload(3, *hiplib.pack_reads([]))
    none = np.zeros(0, np.int32)
    assert _raw(sc, 3, _One, np.zeros(0, hiplib.REFINE_DTYPE), tails=none, begin=none, end=none, at=none) == 0


def _cli(argv, engines=None):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


def test_cli_end_to_end_equals_the_emulations_files(tmp_path):
    """The CLI fixture once on the device, two passes: its files are the oracle's rows and, byte for byte, those of the run on the
    emulation engines; every other file is as without the flag."""
    import emu_adapter_driver
    import emu_anchor_driver
    import emu_driver
    import emu_ends_driver
    import emu_follow_wide_driver
    import emu_motif_driver
    import emu_variant_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver, emu_variant_driver, emu_ends_driver, emu_anchor_driver,
              emu_adapter_driver, emu):
        d.build()
    from emu_refine_engine import EmuRefineEngine
    seqs, _planted = rc.cli_reads()
    d = tmp_path / "in"
    d.mkdir()
    vc.write_fasta(str(d / "reads.fasta"), seqs)
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--gpus", "1"]
    _cli(common + ["-o", str(tmp_path / "plain")])
    _cli(common + ["-o", str(tmp_path / "gpu"), "--refine", "--twopass", "on"])
    _cli(common + ["-o", str(tmp_path / "emu"), "--refine", "--twopass", "off"], [EmuRefineEngine(), EmuRefineEngine()])
    read = lambda p: open(p, "rb").read()      # noqa: E731
    assert not os.path.exists(tmp_path / "plain" / "refined_4.csv")
    others = sorted(f for f in os.listdir(tmp_path / "plain") if f != "topsicle_run.log")
    assert "telolengths_all.csv" in others
    for f in others:
        assert read(tmp_path / "plain" / f) == read(tmp_path / "gpu" / f), f
    for f in ("refined_4.csv", "refine_summary_4.csv"):
        assert read(tmp_path / "gpu" / f) == read(tmp_path / "emu" / f), f
    assert len(rc.check_cli_outputs(str(tmp_path / "gpu"), seqs, "CCCTAA", [4])) >= 20
    assert "refined boundaries:" in open(tmp_path / "gpu" / "topsicle_run.log").read()
