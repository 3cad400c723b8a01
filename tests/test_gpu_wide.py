"""Wide pattern tables (tps_set_patterns_wide: k <= 32 letters, P <= 64 patterns) on the MI355X, everything through the C ABI:
the case matrix of tests/wide_cases.py against oracle/oracle.c, 10 000 x 15 kb reads with every window compared, a narrow table
through both kernels, table switches on resident and borrowed batches, the loud refusals."""
import numpy as np
import pytest

import bam_tools as bt
import oracle_c
import topsicle_oracle as orc
import wide_cases
from topsicle_amd import allsteps, hiplib, seqio, synth

pytestmark = pytest.mark.gpu
FULL = hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS
WIDE = "tps_scan_kernel_wide"


@pytest.fixture(scope="module")
def sc():
    s = hiplib.HipScanner(0)
    yield s
    s.close()


def _collect(sc, slot, prm):
    """dict(results, c_start, c_end, win_off, sums, raw) of the slot's last scan, like the emulation drivers return."""
    res = sc.results(slot).copy()
    out = dict(results=res, win_off=sc.window_offsets(slot))
    if prm.flags & hiplib.F_STEP1:
        out["c_start"], out["c_end"] = sc.batch_trc_counts(slot)
    if prm.flags & hiplib.F_STORE_SUMS:
        out["sums"], _ = sc.window_sums(slot)
    if prm.flags & hiplib.F_STORE_RAW:
        out["raw"], _ = sc.window_raw(slot)
    return out


def _scan(sc, slot, patterns, bases, offsets, prm, tails=None, wide=True):
    (sc.set_patterns_wide if wide else sc.set_patterns)(patterns)
    sc.upload(slot, bases, offsets)
    if tails is not None:
        sc.set_tails(slot, tails)
    sc.scan(slot, prm)
    sc.sync()
    return _collect(sc, slot, prm)


def _same(a, b, gain=True):
    """Two scans of one batch gave the same: every result field, the step-1 counts, and S_w / raw rows of every read that passed
    (the window region of a read that did not pass is never written)."""
    for f in a["results"].dtype.names:
        if f == "gain" and not gain:
            continue
        assert np.array_equal(a["results"][f], b["results"][f]), f
    assert np.array_equal(a["win_off"], b["win_off"])
    for key in ("c_start", "c_end"):
        assert np.array_equal(a[key], b[key]), key
    keep = np.repeat(a["results"]["pass"].astype(bool), np.diff(a["win_off"]))
    assert keep.sum() > 0
    for key in ("sums", "raw"):
        if key in a:
            assert np.array_equal(a[key][keep], b[key][keep]), key


def test_case_matrix_against_the_c_oracle(sc):
    cases = wide_cases.cases()
    picked = cases[:300:5] + cases[300:]
    assert {32, 46, 50, 64} <= {len(c["patterns"]) for c in picked} and {6, 14, 21, 23, 30, 32} <= {len(c["patterns"][0]) for c in picked}
    assert {c["mode"] for c in picked} == {"sums", "raw", "tails", "step1"}
    rng = np.random.default_rng(1)
    windows = 0
    for ci, c in enumerate(picked):
        prm = wide_cases.params_of(c)
        tails = wide_cases.tails_for(c, rng) if c["mode"] == "tails" else None
        bases, offsets = hiplib.pack_reads(c["seqs"])
        out = _scan(sc, ci % 3, c["patterns"], bases, offsets, prm, tails)
        assert sc.kernel_info(ci % 3).startswith(WIDE + " ")
        windows += wide_cases.check_output(c, out, tails)
    print(f"{len(picked)} cases, {windows} windows compared with oracle.c")
    assert len(picked) >= 60 and windows > 20000


def _params(motif, slide, cutoff, flags=FULL):
    return hiplib.make_params(no_bp=1000, min_len=9000, min_count=allsteps.min_count_for_cutoff(cutoff, 1000 / len(motif), 1000),
                              window=100, slide=slide, trimfirst=100, maxlen=20000, flags=flags)


def _assert_equals_float64_pipeline(sc, slot, res, out_ck, sums, win_off, P):
    """tests/test_gpu_configs.py's comparison, for the wide kernel: every window through the per-read checksums, step 1's outcome,
    and the change point against the float64 restatement -- reads the device flagged TPS_RES_TIE resolved as hiplib.resolve_ties does."""
    out, ck = out_ck
    p = res["pass"].astype(bool)
    got = oracle_c.checksums(sums, win_off)
    bad = np.nonzero(got[p] != ck[p, 0])[0]
    print(f"window sums: GPU vs oracle.c checksums on {int(p.sum())} reads ({int(np.diff(win_off)[p].sum())} windows): {len(bad)} differ")
    assert len(bad) == 0, bad[:10]
    assert np.array_equal(res["pass"], out[:, 0])
    assert np.array_equal(res["tail"][p], out[p, 1])
    best = np.where(res["tail"] == 0, res["best_start"], res["best_end"])
    idx = np.where(res["tail"] == 0, res["best_start_idx"], res["best_end_idx"])
    assert np.array_equal(best[p], out[p, 3]) and np.array_equal(idx[p], out[p, 2])
    assert np.array_equal(res["n_win"][p], out[p, 4])
    n_tie = hiplib.resolve_ties(sc, slot, res, P)
    differ = np.nonzero(res["bkp"][p] != out[p, 5])[0]
    print(f"change-point: GPU vs float64 restatement on {int(p.sum())} reads ({n_tie} ties resolved on the host): {len(differ)} disagreements")
    assert len(differ) == 0, (differ[:10], res["bkp"][p][differ[:10]], out[p, 5][differ[:10]])


def test_at_scale_23_letter_motif_every_window(sc):
    """10 000 reads x 15 kb of the 23-letter motif at the reference's defaults (k = 21, P = 46, slide = 23); --cutoff 0.2: at the
    generator's noise a 21-mer survives rarely and the default cutoff passes no read."""
    motif = wide_cases.MOTIFS[23]
    pats = orc.kmer_table(motif, len(motif) - 2)
    assert len(pats) == 46 and hiplib.needs_wide(pats)
    slide, cutoff = len(motif), 0.2
    bases, offsets, _ = synth.make_reads(10000, 15000, motif, seed=20261016)
    prm = _params(motif, slide, cutoff)
    out = _scan(sc, 0, pats, bases, offsets, prm)
    assert sc.kernel_info(0).startswith(WIDE + " ")
    res = out["results"]
    print("reads that pass step 1:", int(res["pass"].sum()))
    assert res["pass"].sum() > 5000
    ref = oracle_c.batch_ck(bases, offsets, pats, len(motif), 1000, 9000, cutoff, 100, slide, 100, 20000, both_tails=False, threads=oracle_c.usable_cores())
    _assert_equals_float64_pipeline(sc, 0, res, ref, out["sums"], out["win_off"], len(pats))
    # raw rows in full on a 500-read slice
    m = 500
    prm_raw = _params(motif, slide, cutoff, FULL | hiplib.F_STORE_RAW)
    out_r = _scan(sc, 1, pats, bases[:offsets[m]], offsets[:m + 1], prm_raw)
    _, ck = oracle_c.batch_ck(bases[:offsets[m]], offsets[:m + 1], pats, len(motif), 1000, 9000, cutoff, 100, slide, 100, 20000,
                              both_tails=False, threads=oracle_c.usable_cores(), want_raw=True)
    p = out_r["results"]["pass"].astype(bool)
    got = oracle_c.checksums(out_r["raw"].reshape(-1), out_r["win_off"] * len(pats))
    assert p.sum() > 200 and np.array_equal(got[p], ck[p, 1])
    keep = np.repeat(p, np.diff(out_r["win_off"]))       # (the window region of a read that did not pass is never written)
    assert np.array_equal(out_r["sums"][keep], out["sums"][:out["win_off"][m]][keep]) and np.array_equal(out_r["raw"][keep].sum(axis=1), out_r["sums"][keep])
    for f in ("pass", "tail", "n_win", "bkp", "best_start", "best_end"):
        assert np.array_equal(out_r["results"][f], res[f][:m]), f


def _nib4_batch(seqs):
    """(nib, src, desc, n_words) of forward-strand BAM records holding `seqs`: the layout tps_reader_next_nib4 gives."""
    nib, src = [], []
    off = 0
    for s in seqs:
        codes = [bt.CODE[c] for c in s] + ([0] if len(s) & 1 else [])
        a = np.array(codes, np.uint8)
        b = ((a[0::2] << 4) | a[1::2]).tobytes()
        pad = ((len(b) + 15) // 16) * 16
        nib.append(b + bytes(pad - len(b)))
        src.append((off, 0, 0))
        off += pad
    bases, offsets = hiplib.pack_reads(seqs)
    seq2, _, desc = seqio.pack_reads_host(bases, offsets)
    return np.frombuffer(b"".join(nib), np.uint8).copy(), np.array(src, hiplib.NIB_SRC_DTYPE), desc.copy(), len(seq2)


def test_at_scale_ragged_reads_16_letter_motif_from_bam_nibbles(sc):
    """2 000 reads of log-normal length (up to 60 kb) of the 16-letter motif (k = 14, P = 32: one pattern too many for the narrow
    table), uploaded as BAM's 4-bit codes."""
    motif = wide_cases.MOTIFS[16]
    pats = orc.kmer_table(motif, 14)
    assert len(pats) == 32 and hiplib.needs_wide(pats)
    slide, cutoff = len(motif), 0.2
    bases, offsets, _ = synth.make_ragged_reads(2000, motif, seed=20261017, n_frac=0.0005)
    seqs = synth.split_reads(bases, offsets)
    nib, src, desc, nw = _nib4_batch(seqs)
    prm = _params(motif, slide, cutoff)
    sc.set_patterns_wide(pats)
    sc.upload_nib4(2, nib, src, desc, nw)
    sc.scan(2, prm)
    sc.sync()
    out = _collect(sc, 2, prm)
    assert sc.kernel_info(2).startswith(WIDE + " ")
    assert out["results"]["pass"].sum() > 300
    ref = oracle_c.batch_ck(bases, offsets, pats, len(motif), 1000, 9000, cutoff, 100, slide, 100, 20000, both_tails=False, threads=oracle_c.usable_cores())
    _assert_equals_float64_pipeline(sc, 2, out["results"], ref, out["sums"], out["win_off"], len(pats))


def test_narrow_table_through_both_kernels(sc):
    """A 15-letter motif at k = 13 (P = 30) scanned through set_patterns and through set_patterns_wide on the same resident batch."""
    motif = "ACGGATGTCTAACTT"
    pats = orc.kmer_table(motif, 13)
    assert len(pats) == 30 and not hiplib.needs_wide(pats)
    bases, offsets, _ = synth.make_reads(512, 12000, motif, seed=5, tract_min=500, tract_max=6000)
    sc.upload(0, bases, offsets)
    for slide in (6, 15):
        prm = _params(motif, slide, 0.3, FULL | hiplib.F_STORE_RAW)
        sc.set_patterns(pats)
        sc.scan(0, prm)
        sc.sync()
        narrow = _collect(sc, 0, prm)
        assert not sc.kernel_info(0).startswith(WIDE)
        sc.set_patterns_wide(pats)
        sc.scan(0, prm)
        sc.sync()
        wide = _collect(sc, 0, prm)
        assert sc.kernel_info(0).startswith(WIDE + " ")
        assert narrow["results"]["pass"].sum() > 100
        for o in (narrow, wide):                           # (which reads take the exact tournament is each kernel's own; the answer is not)
            hiplib.resolve_ties(sc, 0, o["results"], len(pats))
            o["results"]["flags"] = 0
        _same(narrow, wide, gain=False)
        # gain is informational: m / n / P^2 from the same exact integers in both kernels, a handful of float64 roundings apart at most
        assert np.allclose(narrow["results"]["gain"], wide["results"]["gain"], rtol=1e-12, atol=0.0)


def test_table_switches_on_resident_and_borrowed_batches(sc):
    """narrow -> wide -> another wide table of the same k and P with other periods -> narrow, on one resident batch (slide 10: the
    narrow scans run in the hidden sub-slot of the strided scans); then a wide table on a batch borrowed with share.  Every scan
    equals that of a fresh context."""
    rng = np.random.default_rng(9)
    narrow = orc.kmer_table("CCCTAA", 4)
    wide_a = orc.kmer_table("AC" * 10, 16)                                              # P = 4, every even period
    wide_b = ["".join("ACGT"[i] for i in rng.integers(0, 4, 16)) for _ in range(4)]    # P = 4, no period
    reads = []
    for i in range(96):
        tract = ("CCCTAA" * 400, "AC" * 1200, (wide_b[i % 4] + "T") * 150)[i % 3][: int(rng.integers(600, 2400))]
        reads.append(tract + "".join("ACGT"[j] for j in rng.integers(0, 4, int(rng.integers(3000, 9000)))))
    bases, offsets = hiplib.pack_reads(reads)
    prm = hiplib.make_params(min_len=1000, min_count=2, slide=10, flags=FULL | hiplib.F_STORE_RAW)

    def fresh(table):
        with hiplib.HipScanner(0) as f:
            return _scan(f, 0, table, bases, offsets, prm, wide=table is not narrow)

    want = {id(t): fresh(t) for t in (narrow, wide_a, wide_b)}
    sc.upload(5, bases, offsets)
    for table in (narrow, wide_a, wide_b, narrow, wide_b, wide_a, narrow):
        (sc.set_patterns if table is narrow else sc.set_patterns_wide)(table)
        sc.scan(5, prm)
        sc.sync()
        assert sc.kernel_info(5).startswith(WIDE) == (table is not narrow)
        _same(_collect(sc, 5, prm), want[id(table)])
    h = sc.helper(0)
    h.share(5, sc, 5)
    h.set_patterns_wide(wide_a)
    sc.set_patterns_wide(wide_b)
    h.scan(5, prm)
    sc.scan(5, prm)
    h.sync()
    sc.sync()
    _same(_collect(h, 5, prm), want[id(wide_a)])
    _same(_collect(sc, 5, prm), want[id(wide_b)])
    # the one-shot calls scan with the wide table too
    cs, ce = sc.trc_counts(bases, offsets)
    assert np.array_equal(cs, want[id(wide_b)]["c_start"]) and np.array_equal(ce, want[id(wide_b)]["c_end"])


def test_wide_error_paths_are_loud(sc):
    for bad in (["A" * 33], ["ACGT" * 5 + "ACGT"[i % 4] + "ACGT"[i // 4 % 4] + "ACGT"[i // 16 % 4] + "ACGT"[i // 64] for i in range(65)], ["ACGN"]):
        with pytest.raises(hiplib.TopsicleHipError):
            sc.set_patterns_wide(bad)
    pats = orc.kmer_table(wide_cases.MOTIFS[16], 14)
    sc.set_patterns_wide(pats)
    sc.upload(0, *hiplib.pack_reads(["ACGT" * 1000]))
    with pytest.raises(hiplib.TopsicleHipError):
        sc.kmer_followers(0, 15, 2)
    sc.set_patterns_wide(["A"])
    with pytest.raises(hiplib.TopsicleHipError):           # (window - 1) / k > 255
        sc.scan(0, hiplib.make_params(window=300, flags=hiplib.F_WINDOWS))
    sc.set_patterns(orc.kmer_table("CCCTAA", 4))           # ... and the narrow call still refuses what it refused
    with pytest.raises(hiplib.TopsicleHipError):
        sc.set_patterns(pats)
