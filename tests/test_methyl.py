"""`--methyl` without a GPU: the kernel's host emulation against the plain rule on every case of tests/methyl_cases.py (and as a
stand-alone program under the sanitizers), the native reader's aux walk against expectations written out by hand (and the same as a
program), the one extension of batch.run_analysis, and the CLI on the emulation engines.  tests/test_gpu_methyl.py runs the same
cases on the GPU."""
import csv
import os
import subprocess

import numpy as np
import pytest

import bam_tools
import emu_methyl_driver as emu
import methyl_cases as mc
import methyl_oracle as mo
from topsicle_amd import analyses, batch, hiplib, methyl, seqio
from topsicle_amd import main as cli


def _run(c, idx=None, **kw):
    pick = (lambda x: list(x)) if idx is None else (lambda x: [x[i] for i in idx])
    return emu.mod_profile(pick(c.reads), pick(c.tails), pick(c.begin), pick(c.end), pick(c.origin), *c.lists(idx), **dict(c.kw(), **kw))


@pytest.mark.parametrize("name", mc.names())
def test_every_case_equals_the_oracle(name):
    mc.assert_equal(_run(mc.case(name)), name)


def test_a_moved_batch_and_a_subset_of_the_reads():
    c = mc.case("mixed")
    for shift in (1, 2, 3):
        mc.assert_equal(_run(c, base_shift=shift), "mixed")
    idx = [i for i in range(len(c.reads)) if i % 3 != 1]
    mc.assert_equal(_run(c, idx), "mixed", idx)
    mc.assert_equal(_run(mc.case("regions"), [4, 2, 9]), "regions", [4, 2, 9])


def test_the_cases_cover_what_they_are_for():
    rows, bins = mc.expected("mixed")
    assert (rows["flags"] & hiplib.MOD_BAD).any() and (rows["c_total"] == 0).any() and (rows["called"] > 0).any() and (rows["off_context"] > 0).any()
    rows, bins = mc.expected("entry_counts")
    assert sorted(set(rows["entries"].tolist())) == [0, 1, 2, 4, 5, 63, 64, 65, 70, 129] and rows["beyond"].tolist()[-5:] == [0, 1, 2, 3, 70]
    rows, bins = mc.expected("largest")
    assert bins[2]["called"].tolist() == [2048, 2048, 2048, 2048, 0] and bins[2]["sum"].max() == 2048 * 255
    rows, bins = mc.expected("regions")
    assert (bins[0, :2]["cpg"] > 0).all()                      # bins in front of the origin are filled: t - origin < 0
    rows, bins = mc.expected("seams")
    assert rows["cpg"].tolist()[0:12:4] == [2, 1, 2] and rows["cpg"].tolist()[2:12:4] == [2, 1, 2]      # CG and Cg across a word seam; CN is none
    assert rows["cpg"].tolist()[24:28] == [2, 1, 2, 1]         # ... across the 64th and 65th word of the region
    rows, bins = mc.expected("long")
    assert rows["in_region"][0] > 10 and rows["entries"][0] > 10 * rows["in_region"][0]


class _One:
    """The good call of the refusal tests: one read of 120 letters, two entries."""
    reads, tails, begin, end, origin, mod_off, delta, prob = ["ACGT" * 30], [0], [0], [100], [50], [0, 2], [0, 0], [1, 2]


def emu_refusal(reads, kw, good=_One):
    """The emulation's message for the good call changed by `kw`."""
    k = dict(kw)
    n = len(reads)
    nb = k.get("nb0", 2) + k.get("nb1", 8)
    lens = (k.pop("n_reads", n), len(good.delta), k.pop("rows_len", n), k.pop("bins_len", n * nb))
    args = {f: k.pop(f, getattr(good, f)) for f in ("tails", "begin", "end", "origin", "mod_off")}
    with pytest.raises(hiplib.TopsicleHipError) as e:
        emu.mod_profile(reads, args["tails"], args["begin"], args["end"], args["origin"], args["mod_off"], good.delta, good.prob, lens=lens, **k)
    return str(e.value)


@pytest.mark.parametrize("kw, code, text", mc.REFUSALS)
def test_refusals(kw, code, text):
    msg = emu_refusal(_One.reads, kw)
    assert code + ":" in msg and text in msg
    rows, bins = emu.mod_profile(_One.reads, _One.tails, _One.begin, _One.end, _One.origin, _One.mod_off, _One.delta, _One.prob)
    assert rows["c_total"][0] == 30 and rows["in_region"][0] == 2 and rows["off_context"][0] == 0 and bins[0]["called"].tolist() == [0, 2] + [0] * 8


def test_region_cap_and_empty_batch():
    kw, code, text = mc.LONG_REFUSAL
    reads = ["ACGT" * 4100] * 2
    two = dict(tails=[0, 1], origin=[0, 0], mod_off=[0, 1, 2], w=4096, nb0=0, nb1=5)
    msg = emu_refusal(reads, dict(two, **kw))
    assert code + ":" in msg and text in msg
    rows, _ = emu.mod_profile(reads, [0, 1], [0, 16], [16384, 1 << 30], [0, 0], [0, 1, 2], [0, 0], [1, 2], w=4096, nb0=0, nb1=5)      # 16 384 each: end is clamped first
    assert rows["cpg"].tolist() == [4096, 4096]
    rows, bins = emu.mod_profile([], [], [], [], [], [0], [], [])
    assert len(rows) == 0 and bins.shape == (0, 10)


def _case_file(path):
    with open(path, "w") as f:
        for name in mc.names():
            c = mc.case(name)
            k = c.kw()
            f.write(f"mcase {k['w']} {k['nb0']} {k['nb1']} {k['hi']} {k['lo']} {len(c.reads)}\n")
            for s, t, b, e, o, (d, p) in zip(c.reads, c.tails, c.begin, c.end, c.origin, c.ents):
                f.write(f"{t} {b} {e} {o} {s or '-'} {len(d)} " + " ".join(f"{x} {y}" for x, y in zip(d, p)) + "\n")


def test_emulation_as_a_program_under_the_sanitizers(tmp_path):
    exe = emu.build_main()
    _case_file(tmp_path / "cases.txt")
    for argv in ([exe, str(tmp_path / "cases.txt")], [exe]):
        out = subprocess.run(argv, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.strip().startswith("ok") and "runtime error" not in out.stderr, (out.stdout[-2000:], out.stderr[-4000:])
    assert f"ok {len(mc.names())} cases" in subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True).stdout


# ---- the aux walk
def _native(text, spans, lens, idx, code="m", cap=None):
    lib = seqio._load_io()
    t = np.frombuffer(text, np.uint8)
    idx = np.ascontiguousarray(idx, np.int64)
    st, md, off = np.full(len(idx), -9, np.int32), np.full(len(idx), 9, np.uint8), np.full(len(idx) + 1, -9, np.int64)
    cap = 256 if cap is None else cap
    d, p = np.full(cap + 1, 77, np.uint32), np.full(cap + 1, 77, np.uint8)
    got = lib.tps_bam_mods_spans(t.ctypes.data, len(t), spans.ctypes.data, lens.ctypes.data, idx.ctypes.data, len(idx), code.encode(), st.ctypes.data, md.ctypes.data,
                                 off.ctypes.data, d.ctypes.data, p.ctypes.data, cap)
    return got, st, md, off, d, p


def test_aux_walk_equals_the_expectations_and_the_oracle():
    text, spans, lens = mc.aux_window()
    assert spans[-1][3] + 60 + len(mc.AUX_CASES[-1][1]) == len(text)                 # the last record ends where the window ends
    for code in "mh":
        idx = [i for i, c in enumerate(mc.AUX_CASES) if c[3] == code]
        got, st, md, off, d, p = _native(text, spans, lens, idx, code)
        assert got == sum(len(mc.AUX_CASES[i][2][2]) for i in idx) and off[0] == 0 and off[-1] == got
        for j, i in enumerate(idx):
            name, block, want, _code = mc.AUX_CASES[i]
            mine = (int(st[j]), int(md[j]), d[off[j]:off[j + 1]].tolist(), p[off[j]:off[j + 1]].tolist())
            assert mine == want, name
            assert tuple(mo.record_mods(block, 60, code)) == want, name
    names = [c[0] for c in mc.AUX_CASES]
    for must in ("every_type_in_front", "two_codes_first", "two_codes_swapped", "second_group", "base_n", "minus_strand", "chebi_only", "empty_list", "ml_one_short",
                 "count_two_to_32", "mn_differs", "ml_without_mm", "at_the_end_of_the_window"):
        assert must in names
    assert {c[2][0] for c in mc.AUX_CASES} == {0, 1, 2, 3, 4}


def test_aux_walk_capacity_and_bad_spans():
    text, spans, lens = mc.aux_window()
    idx = [i for i, c in enumerate(mc.AUX_CASES) if c[3] == "m"]
    total = _native(text, spans, lens, idx)[0]
    got, st, md, off, d, p = _native(text, spans, lens, idx, cap=total - 1)           # one too small: -2 and nothing written
    assert got == -2 and (st == -9).all() and (md == 9).all() and (off == -9).all() and (d == 77).all() and (p == 77).all()
    got, st, md, off, d, p = _native(text, spans, lens, idx, cap=total)
    assert got == total and d[total] == 77 and p[total] == 77
    lib = seqio._load_io()
    for col, value in ((0, 20), (0, len(text) + 50), (3, len(text) - 10), (3, -5)):
        bad = spans.copy()
        bad[3, col] = value
        assert _native(text, bad, lens, [3])[0] == -1 and b"span" in lib.tps_io_last_error()
    cut = text[:-3]                                                                   # the last record's block_size points past the window
    assert _native(cut, spans, lens, [len(spans) - 1])[0] == -1
    assert _native(text, spans, lens, [0], code="M")[0] == -1 and b"lower-case" in lib.tps_io_last_error()
    got, st, *_ = _native(text, spans, lens, [])
    assert got == 0


def test_aux_walk_as_a_program_under_the_sanitizers(tmp_path):
    exe = emu.build_mods_main()
    text, spans, lens = mc.aux_window()
    (tmp_path / "text.bin").write_bytes(text)
    with open(tmp_path / "spans.txt", "w") as f:
        f.write("m\n" + "".join(f"{a} {b} {c} {d} {n}\n" for (a, b, c, d), n in zip(spans.tolist(), lens.tolist())))
    out = subprocess.run([exe, str(tmp_path / "text.bin"), str(tmp_path / "spans.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, (out.stdout[-2000:], out.stderr[-4000:])
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "ok" and "-2, nothing written" in lines[0]
    for line, (name, block, _want, _code) in zip(lines[1:-1], mc.AUX_CASES):
        status, mode, deltas, probs = mo.record_mods(block, 60, "m")
        assert line == " ".join([str(status), str(mode)] + [f"{a}:{b}" for a, b in zip(deltas, probs)]), name


def test_thresholds_are_the_bytes_the_probabilities_give():
    assert methyl.thresholds(0.8, 0.2) == (205, 50) == mo.thresholds(0.8, 0.2)
    assert (204 + 0.5) / 256 < 0.8 <= (205 + 0.5) / 256 and (50 + 0.5) / 256 <= 0.2 < (51 + 0.5) / 256
    assert methyl.MethylSpec().hi == 205 and methyl.MethylSpec().lo == 50
    assert methyl.fraction(10, 4, 3, 1, 1) == 0.75 and methyl.fraction(10, 4, 3, 1, 0) == 0.3 and methyl.fraction(0, 0, 0, 0, 0) is None


# ---- the batch driver
def test_mods_of_a_batch_and_their_subsets(tmp_path):
    reads, truth = mc.cli_bam_reads(n=12, L=3000)
    bam_tools.write_bam(str(tmp_path / "r.bam"), reads)
    pool = seqio.BufferPool(2, 1 << 16, 256)
    (pb,) = list(seqio.read_batches_packed(str(tmp_path / "r.bam"), pool))
    wanted = np.array([i % 2 == 0 for i in range(12)])
    mods = seqio.bam_mods(pb, wanted)
    pb.release()
    again = seqio.bam_mods(pb, wanted)                         # the record text outlives the staging buffers
    for a, b in zip((mods.status, mods.mode, mods.mod_off, mods.delta, mods.prob), (again.status, again.mode, again.mod_off, again.delta, again.prob)):
        assert np.array_equal(a, b)
    for i, (kind, _tract, deltas, probs, flag_mode) in enumerate(truth):
        mine = mods.delta[mods.mod_off[i]:mods.mod_off[i + 1]].tolist(), mods.prob[mods.mod_off[i]:mods.mod_off[i + 1]].tolist()
        if wanted[i] and kind not in ("none", "malformed"):
            assert mods.status[i] == 0 and mine == (deltas, probs) and mods.mode[i] == (flag_mode == "?")
        else:
            assert mine == ([], []) and mods.status[i] == (0 if not wanted[i] else 1 if kind == "none" else 3)
    sub = mods[np.array([8, 0, 4])]
    assert len(sub) == 3 and sub.mod_off[0] == 0 and sub.mod_off[-1] == len(sub.delta) == len(sub.prob)
    for j, i in enumerate((8, 0, 4)):
        assert sub.delta[sub.mod_off[j]:sub.mod_off[j + 1]].tolist() == truth[i][2] and sub.prob[sub.mod_off[j]:sub.mod_off[j + 1]].tolist() == truth[i][3]
    fq = seqio.bam_mods(seqio.RecordBatch.from_records([seqio.Record("a", "a", "ACGT", "IIII")]), np.array([True]))
    assert fq.status.tolist() == [5] and len(fq.delta) == 0


def test_run_analysis_hands_the_records_to_a_spec_that_needs_them():
    seen = {}

    class Extra:
        def __init__(self, v):
            self.v = v

        def __getitem__(self, sel):
            return Extra(self.v[sel])

    class Spec(analyses.BoundaryAnalysis):
        needs_records = True

        def regions(self, res, prm, recs):
            seen["recs"] = recs
            n = len(res)
            return np.zeros(n, np.int32), np.arange(n, dtype=np.int32), Extra(np.arange(n) * 10)

        def empty(self, n):
            return np.full(n, -1),

        def launch(self, eng, slot, tails, begin, end, extra):
            seen["launch"] = (tails.tolist(), end.tolist(), extra.v.tolist())
            return extra.v + 1,

        def sink(self, recs, res, out):
            seen["out"] = out.tolist()

    res = np.zeros(5, hiplib.RESULT_DTYPE) if hasattr(hiplib, "RESULT_DTYPE") else np.zeros(5, [("tail", "u1")])
    res["tail"] = 1
    recs = object()
    batch.run_analysis(Spec(), None, "eng", 0, recs, res)
    assert seen["recs"] is recs and seen["launch"] == ([0, 1, 1, 1, 1], [0, 1, 2, 3, 4], [0, 10, 20, 30, 40]) and seen["out"] == [1, 11, 21, 31, 41]
    batch.run_analysis(Spec(), None, "eng", 1, recs, res, slot_index=np.array([3, 1]))
    assert seen["launch"] == ([1, 1], [3, 1], [30, 10]) and seen["out"] == [-1, 11, -1, 31, -1]
    batch.run_analysis(Spec(), None, None, 1, recs, res)
    assert seen["out"] == [-1] * 5


# ---- the CLI on the emulation engines
@pytest.fixture(scope="module")
def engines():
    import emu_adapter_driver
    import emu_anchor_driver
    import emu_driver
    import emu_ends_driver
    import emu_follow_wide_driver
    import emu_motif_driver
    import emu_refine_driver
    import emu_variant_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver, emu_variant_driver, emu_ends_driver, emu_anchor_driver, emu_adapter_driver,
              emu_refine_driver, emu):
        d.build()
    from emu_methyl_engine import EmuMethylEngine
    return [EmuMethylEngine(), EmuMethylEngine()]


@pytest.fixture(scope="module")
def bam_reads():
    return mc.cli_bam_reads()


def _cli(argv, engines):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


def _read(path):
    return open(path, "rb").read()


COMMON = ["--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4"]


def check_methyl_run(outdir, reads, truth, k=4):
    """What the issue asks of methyl_{k}.csv on the end-to-end fixture."""
    rows = mc.check_cli_outputs(str(outdir), reads, truth, [k])
    kinds = {r[0]: t[0] for r, t in zip(reads, truth)}
    assert len(rows) >= 30
    for r in rows:
        kind = kinds[r["readID"]]
        assert r["tags"] == {"high": "ok", "low": "ok", "none": "none", "malformed": "malformed"}[kind], r
        if kind in ("high", "low"):
            assert int(r["called"]) > 10 and float(r["meth_fraction"]) == (1.0 if kind == "high" else 0.0), r
    assert {"none", "malformed", "ok"} <= {r["tags"] for r in rows} and {"forward", "reverse"} <= {r["tail"] for r in rows}
    assert {"explicit", "implicit"} <= {r["mode"] for r in rows}
    prof = list(csv.DictReader(open(outdir / f"methyl_profile_{k}.csv")))
    assert [int(p["bin"]) for p in prof] == list(range(-2, 8)) and sum(int(p["called"]) for p in prof[2:]) == sum(int(r["called"]) for r in rows if r["tags"] == "ok")
    return rows


def test_methyl_end_to_end(tmp_path, engines, bam_reads):
    reads, truth = bam_reads
    d = tmp_path / "in"
    d.mkdir()
    bam_tools.write_bam(str(d / "reads.bam"), reads)
    common = ["-i", str(d)] + COMMON
    _cli(common + ["-o", str(tmp_path / "plain")], engines)
    assert sum(len(getattr(e, "methyl_calls", [])) for e in engines) == 0                  # without the flag nothing is looked at
    _cli(common + ["-o", str(tmp_path / "meth"), "--methyl"], engines)
    assert sum(len(getattr(e, "methyl_calls", [])) for e in engines) >= 1
    check_methyl_run(tmp_path / "meth", reads, truth)
    others = sorted(f for f in os.listdir(tmp_path / "plain") if f != "topsicle_run.log")
    assert "telolengths_all.csv" in others
    assert sorted(f for f in os.listdir(tmp_path / "meth") if f != "topsicle_run.log" and not f.startswith("methyl")) == others
    for f in others:
        assert _read(tmp_path / "plain" / f) == _read(tmp_path / "meth" / f), f
    log = open(tmp_path / "meth" / "topsicle_run.log").read()
    assert "methylation: " in log and "none 2, nogroup 0, malformed 1" in log and "median meth_fraction" in log


def test_methyl_with_ends_and_several_telophrase(tmp_path, engines, bam_reads):
    reads, truth = bam_reads
    d = tmp_path / "in"
    d.mkdir()
    bam_tools.write_bam(str(d / "reads.bam"), reads)
    common = ["-i", str(d), "--pattern", "CCCTAA", "--minSeqLength", "5000", "--cutoff", "0.4", "--telophrase", "4", "5", "--ends", "--endminreads", "1",
              "--endminkmers", "10"]
    _cli(common + ["-o", str(tmp_path / "ends")], engines)
    _cli(common + ["-o", str(tmp_path / "both"), "--methyl", "--methylbin", "250", "--methylbins", "6", "--methyltract", "1", "--refine"], engines)
    for k in (4, 5):
        rows = mc.check_cli_outputs(str(tmp_path / "both"), reads, truth, [k], bin_w=250, bins=6, tract=1)
        end_reads = list(csv.DictReader(open(tmp_path / "both" / f"end_reads_{k}.csv")))
        assert [r["readID"] for r in rows] == [r["readID"] for r in end_reads]              # one to one
        groups = list(csv.DictReader(open(tmp_path / "both" / f"ends_{k}.csv")))
        mine = list(csv.DictReader(open(tmp_path / "both" / f"methyl_ends_{k}.csv")))
        assert [g["end"] for g in groups] == [m["end"] for m in mine] and [g["reads"] for g in groups] == [m["reads"] for m in mine] and len(mine) >= 1
        assert sum(int(m["called"]) for m in mine) == sum(int(r["called"]) for r, e in zip(rows, end_reads) if r["tags"] == "ok" and e["end"] != "0")
    for f in os.listdir(tmp_path / "ends"):
        if f != "topsicle_run.log":
            assert _read(tmp_path / "ends" / f) == _read(tmp_path / "both" / f), f


def test_fastq_reads_are_untagged_and_a_run_without_bam_ends_with_one_message(tmp_path, engines, bam_reads, capsys):
    reads, truth = bam_reads
    d = tmp_path / "in"
    d.mkdir()
    bam_tools.write_bam(str(d / "a.bam"), reads)
    bam_tools.write_fastq(str(d / "b.fastq"), [(name, s, q) for name, _f, s, q, _c, _t in reads])
    _cli(["-i", str(d), "-o", str(tmp_path / "two")] + COMMON + ["--methyl"], engines)
    rows = list(csv.DictReader(open(tmp_path / "two" / "methyl_4.csv")))
    a, b = [r for r in rows if r["file"] == "a"], [r for r in rows if r["file"] == "b"]
    assert len(a) == len(b) >= 30 and [r["readID"] for r in a] == [r["readID"] for r in b]
    assert all(r["tags"] == "untagged" and r["meth_fraction"] == "" and r["cpg"] == "" for r in b) and sum(r["tags"] == "ok" for r in a) >= 30
    for argv in (["-i", str(d / "b.fastq")], ["-i", str(tmp_path / "no_such_input")]):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            _cli(argv + ["-o", str(tmp_path / "none")] + COMMON + ["--methyl"], engines)
        assert e.value.code == 2 and capsys.readouterr().out.count("--methyl needs BAM input") == 1
        assert not os.path.exists(tmp_path / "none" / "telolengths_all.csv")


def test_bad_methyl_flags_end_the_run_with_one_message(tmp_path, engines, capsys):
    for extra in (["--methylbin", "15"], ["--methylbin", "4097"], ["--methylbins", "0"], ["--methyltract", "-1"], ["--methylbins", "63"], ["--methylbin", "4096"],
                  ["--methylhigh", "0.2"], ["--methyllow", "-0.1"], ["--methylhigh", "1.5"], ["--methylhigh", "1.0"], ["--methyllow", "0.0"], ["--methylcode", "mh"],
                  ["--methylcode", "M"]):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            _cli(["-i", str(tmp_path / "no_such_input"), "-o", str(tmp_path / "out"), "--pattern", "CCCTAA", "--override", "--methyl"] + extra, engines)
        assert e.value.code == 2, extra
        out = capsys.readouterr().out
        assert out.count("--methyl needs") == 1 and "BAM input" not in out, extra
        assert not os.path.exists(tmp_path / "out" / "telolengths_all.csv")
