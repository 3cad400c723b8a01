"""Series of more than 3 301 windows per read (tests/long_series.py) on the MI355X: every row on its clean and its dirty batch --
the launched kernel by its exact name, every output against the C oracle, a second scan of the cached plan byte-identical --, the
strided scans on either side of tps_stride_kernel's LDS limit (6 144 windows in LDS, 6 145 read back from HBM) against the oracle
and against the generic kernel, a slot that goes short batch -> long batch -> short batch, the standalone entry points on a long
batch, the refusal of more than 500 000 windows per read, and the pipeline with --maxlengthtelo raised.  The emulation half is
tests/test_long_series.py."""
import os
import zlib

import numpy as np
import pytest

import cli_cases
import kernel_matrix as km
import long_series as ls
import test_gpu_kernel_matrix as tgkm
import test_gpu_wide_paths as tgwp
import test_long_series as tls
import test_ref_cli_differential as trcd
import wide_path_rows as wp
from topsicle_amd import hiplib
from topsicle_amd import main as cli

pytestmark = pytest.mark.gpu
FIELDS = ("pass", "tail", "n_win", "bkp", "best_start", "best_end", "best_start_idx", "best_end_idx", "flags")


@pytest.fixture(scope="module")
def sc():
    s = hiplib.HipScanner(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def generic_sc():
    """A context whose strided slides keep the generic kernel (debug option no_stride)."""
    s = hiplib.HipScanner(0)
    s.debug_option("no_stride", 1)
    yield s
    s.close()


def _scan_checked(sc, slot, row, reads, dirty, tag, name=None):
    out, info = tgkm.gpu_scan(sc, slot, row, reads, twice=True)
    assert info.split(" lds=")[0] == (name or row.expected(dirty)), (row.id, tag, info)
    km.check_scan(out, row, reads, tag)
    return out


# --------------------------------------------------------------------------------------------- the rows
@pytest.mark.parametrize("row", tls.NARROW, ids=lambda r: r.id)
def test_row(sc, row):
    clean, batch = ls.batches(row)
    a = _scan_checked(sc, 0, row, clean, False, "clean")
    b = _scan_checked(sc, 1, row, batch, True, "dirty")
    shared = min(2, len(clean))
    lo = (len(batch) - shared) // 2
    km.same_outputs(a, b, np.arange(shared), np.arange(lo, lo + shared), row.id + " clean reads in a dirty batch")
    if row is not ls.DEEP:
        names = ls.reads_of(row)[3]
        if "palindrome" in names:
            assert a["results"]["flags"][names["palindrome"]] & hiplib.RES_TIE, "an exact tie must be flagged"


@pytest.mark.parametrize("row", ls.WIDE_ROWS, ids=lambda r: r.id)
def test_row_wide(sc, row):
    prm = row.params()
    for slot, reads in enumerate(ls.wide_reads(row)):
        out, info = tgwp.gpu_scan(sc, slot, row, reads, prm, times=2)
        assert info.startswith(wp.WIDE + " lds="), info
        assert wp.check_scan(out, row, reads, prm) > 30000


# --------------------------------------------------------------------------------------------- strided scans
def _same_as_generic(a, b, reads, row, tag):
    """A strided scan against the generic kernel's scan of the same batch: every result field but the gain (a float the two kernels
    round differently), the step-1 counts, every S_w and every raw byte."""
    for f in FIELDS:
        assert np.array_equal(a["results"][f], b["results"][f]), (tag, f)
    assert np.array_equal(a["win_off"], b["win_off"]) and a["sums"].tobytes() == b["sums"].tobytes(), (tag, "sums")
    assert np.array_equal(a["c_start"], b["c_start"]) and np.array_equal(a["c_end"], b["c_end"]), (tag, "step-1")
    if row.raw:
        assert a["raw"].tobytes() == b["raw"].tobytes(), (tag, "raw")


@pytest.mark.parametrize("fam, slide, base, m", ls.STRIDED, ids=[f"{f}_s{s}" for f, s, _, _ in ls.STRIDED])
def test_strided_scans_on_either_side_of_the_lds_limit(sc, generic_sc, fam, slide, base, m):
    """One slot: the 6 144-window batch (the series in LDS: the largest dynamic-LDS launch of tps_stride_kernel), the 6 145-window
    batch (the series read back from HBM), and the first again.  At twice the base slide also with the raw rows copied
    (no_inline_rows) instead of stored by the tiles."""
    row = ls.stride_row(fam, slide)
    in_lds, in_hbm = ls.stride_batches(row)
    name = ls.stride_name(fam, base, m)
    want = {id(reads): tgkm.gpu_scan(generic_sc, 0, row, reads)[0] for reads in (in_lds, in_hbm)}
    assert generic_sc.kernel_info(0).split(" lds=")[0] == km.GENERIC
    for no_inline in ((0, 1) if m == 2 else (0,)):
        sc.debug_option("no_inline_rows", no_inline)
        try:
            outs = []
            for reads in (in_lds, in_hbm, in_lds):
                tag = f"{row.id} max_nwin {max(ls.nwin(row, x) for x in reads)} no_inline_rows={no_inline}"
                out = _scan_checked(sc, 1, row, reads, False, tag, name=name)
                _same_as_generic(out, want[id(reads)], reads, row, tag)
                outs.append(out)
            idx = np.arange(len(in_lds))
            km.same_outputs(outs[0], outs[2], idx, idx, row.id + " LDS -> HBM -> LDS")
        finally:
            sc.debug_option("no_inline_rows", 0)


# --------------------------------------------------------------------------------------------- slot reuse
@pytest.mark.parametrize("rid, dirty", [("long_p_s6", False), ("long_p_s6", True), ("long_sor_s6", False), ("long_sor_s6", True)])
def test_slot_goes_short_long_short(sc, rid, dirty):
    """The scratch, sum and row buffers of a slot grow for the long batch and are reused by the short one after it."""
    row = ls.BY_ID[rid]
    short = ls.short_batch(row)
    assert max(map(len, short)) < 3000
    long_ = ls.batches(row)[1 if dirty else 0]
    a = _scan_checked(sc, 2, row, short, False, "short")
    _scan_checked(sc, 2, row, long_, dirty, "long")
    b = _scan_checked(sc, 2, row, short, False, "short again")
    idx = np.arange(len(short))
    km.same_outputs(a, b, idx, idx, rid + " short batch before and after the long one")
    assert a["results"]["gain"].tobytes() == b["results"]["gain"].tobytes()


# --------------------------------------------------------------------------------------------- standalone entry points
def test_standalone_entry_points_agree_with_the_fused_scan(sc, tmp_path):
    row = ls.BY_ID["long_r_s6"]
    reads = ls.batches(row)[0]
    out = _scan_checked(sc, 3, row, reads, False, "fused")
    res, sums, win_off = out["results"], out["sums"], out["win_off"]
    assert res["pass"].all()
    bases, offsets = hiplib.pack_reads(reads)
    P = len(row.patterns)
    cs, ce = sc.trc_counts(bases, offsets, row.no_bp)
    assert np.array_equal(cs, out["c_start"]) and np.array_equal(ce, out["c_end"])
    s2, wo2, raw2 = sc.window_counts(bases, offsets, res["tail"].astype(np.uint8), row.W, row.s, row.t, row.M, raw=True)
    assert np.array_equal(wo2, win_off) and s2.tobytes() == sums.tobytes() and raw2.tobytes() == out["raw"].tobytes()
    b2, _ = sc.binseg_l2(sums, win_off, P, row.jump, row.min_size)
    assert np.array_equal(b2, out["bkp_resolved"])
    # (the one-shot calls used scratch slots of their own: slot 3 still holds the fused scan)
    nw = np.diff(win_off)
    longest, shortest = int(np.argmax(nw)), int(np.argmin(np.where(nw > 0, nw, nw.max())))
    assert nw[longest] > 10000 and nw[shortest] == 1
    got = sc.read_sums(3, longest, int(nw[longest]))
    assert got.tobytes() == sums[win_off[longest]:win_off[longest + 1]].tobytes()
    raw = out["raw"]
    sel = np.array(sorted((longest, shortest)), np.int64)
    want = b"".join(raw[win_off[i]:win_off[i + 1]].tobytes() for i in sel)
    fd = os.open(str(tmp_path / "rows.bin"), os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o600)
    try:
        nbytes, crc = sc.raw_to_fd(3, sel, fd, 0)
        assert nbytes == len(want) == int(nw[sel].sum()) * P and os.pread(fd, len(want) + 1, 0) == want and crc == zlib.crc32(want)
    finally:
        os.close(fd)


# --------------------------------------------------------------------------------------------- refusal
def test_more_than_500000_windows_are_refused_and_the_slot_scans_on(sc):
    row = km.Row("long_refused", "p", s=1, M=600000, kernel=km.GENERIC)
    rng = np.random.default_rng(12)
    seq = km._tract("CCCTAA", 2000, rng) + km._rand(500400 - 2000, rng)
    assert len(seq) > 500300 and ls.nwin(row, seq) > 500000
    if sc.patterns != row.patterns:
        sc.set_patterns(row.patterns)
    sc.upload(4, *hiplib.pack_reads([seq, seq[:5000]]))
    with pytest.raises(hiplib.TopsicleHipError, match="too many windows per read") as e:
        sc.scan(4, row.params())
    assert wp.error_code(e.value) == wp.E_CAPACITY, str(e.value)
    ok = ls.BY_ID["long_p_s6"]
    _scan_checked(sc, 4, ok, ls.batches(ok)[0], False, "after the refusal")


# --------------------------------------------------------------------------------------------- the pipeline
def _cli(argv):
    try:
        cli.main(argv)
    except SystemExit as e:
        return e.code if e.code is not None else 0
    return None


def test_pipeline_stores_boundaries_beyond_20000_on_gpu(tmp_path):
    tls.check_pipeline(lambda argv: _cli(argv + ["--gpus", "1"]), tmp_path)


@pytest.mark.parametrize("seed", cli_cases.LONG_SEEDS)
def test_recorded_long_cases_on_gpu(seed, tmp_path, gold_dir):
    import json
    rec = json.load(open(os.path.join(gold_dir, "reference_long_runs.json")))
    rows = trcd.replay_long_case(seed, rec, str(tmp_path / "case"), lambda argv: _cli(argv + ["--gpus", "1"]))
    assert rows and max(int(r[4]) for r in rows) > 20000
