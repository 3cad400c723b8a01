"""Every byte the library hands out is written by somebody, on the MI355X: each call runs twice, its output and scratch buffers
filled beforehand with 0x5A and then with 0xA5 (debug option "poison", include/topsicle_hip.h), and everything it returns must be
byte-identical between the two runs -- no masking -- and equal to its oracle.  A byte that differs is a byte nobody wrote, or a
scratch word read before it was written.  The scan rows are those of the kernel matrix (tests/kernel_matrix.py) on their dirty
batches; the contract for reads that do not pass is held on the seven-read batch of tests/poison_cases.py; every other call runs the
first cases of its own case module against that module's oracle."""
import os
import zlib

import numpy as np
import pytest

import anchor_cases as ac
import ends_cases as ec
import kernel_matrix as km
import motif_cases as mc
import oracle_c as occ
import poison_cases as pc
import test_gpu_bam as tgb
import test_gpu_kernel_matrix as tgkm
import test_gpu_wide_paths as tgwp
import topsicle_oracle as orc
import tract_cases as tc
import variant_cases as vc
import wide_overview_checks as chk
import wide_path_rows as wp
from packfmt import np_pack
from topsicle_amd import allsteps, hiplib

pytestmark = pytest.mark.gpu
FILLS = (0x5A, 0xA5)


@pytest.fixture(scope="module")
def sc():
    s = hiplib.HipScanner(0)
    yield s
    s.close()


def _same(a, b, where="result"):
    """Byte identity of everything a call returned: arrays by dtype, shape and bytes, containers member by member."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, where
        if a.tobytes() != b.tobytes():
            x = np.frombuffer(a.tobytes(), np.uint8)
            y = np.frombuffer(b.tobytes(), np.uint8)
            bad = np.nonzero(x != y)[0]
            raise AssertionError(f"{where}: {len(bad)} of {len(x)} bytes follow the fill (itemsize {a.dtype.itemsize}), first at byte "
                                 f"{bad[:6].tolist()}: {x[bad[:6]].tolist()} under 0x5A, {y[bad[:6]].tolist()} under 0xA5")
    elif isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), where
        for key in a:
            _same(a[key], b[key], f"{where}[{key!r}]")
    elif isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{i}]")
    else:
        assert a == b, (where, a, b)


def twice(sc, call):
    """call() with every output and scratch buffer filled with 0x5A beforehand, and again with 0xA5: all it returns must be the
    same bytes.  Returns the second result, for the oracle."""
    outs = []
    try:
        for fill in FILLS:
            sc.debug_option("poison", fill)
            outs.append(call())
    finally:
        sc.debug_option("poison", 0)
    _same(outs[0], outs[1])
    return outs[1]


# --------------------------------------------------------------------------------------------- narrow scans
@pytest.mark.parametrize("row", km.ROWS, ids=lambda r: r.id)
def test_kernel_matrix_row_on_its_dirty_batch(sc, row):
    _, batch, _ = tgkm._batches(row)
    out, info = twice(sc, lambda: tgkm.gpu_scan(sc, 0, row, batch))
    assert info.split(" lds=")[0] == row.expected(True), info
    km.check_scan(out, row, batch, "dirty batch under poison")


STRIDED = [("r", 12, False, "tps_scan_kernel_s6r every 2nd window"),        # clean batch, P % 4 == 0: the tiles store every 2nd row themselves
           ("r", 12, True, "tps_scan_kernel_s6r every 2nd window"),         # dirty batch: the rows are copied
           ("r", 15, True, "tps_scan_kernel_s5r every 3rd window"),
           ("so", 10, True, "tps_scan_kernel_s5so every 2nd window")]


@pytest.mark.parametrize("fam, slide, dirty, kernel", STRIDED, ids=[f"{f}_s{s}_{'dirty' if d else 'clean'}" for f, s, d, _ in STRIDED])
def test_strided_scans(sc, fam, slide, dirty, kernel):
    """A slide that is a multiple of a fused kernel's: the base scan runs in a hidden slot that borrows the batch, its step-1 counts
    are borrowed back, and at twice the base slide a clean batch's raw rows are stored straight into this scan's layout."""
    row = km.Row(f"{fam}_s{slide}", fam, s=slide, filt=True)
    clean, batch, _ = tgkm._batches(row)
    reads = batch if dirty else clean
    out, info = twice(sc, lambda: tgkm.gpu_scan(sc, 1, row, reads, twice=True))
    assert info.split(" lds=")[0] == kernel, info
    km.check_scan(out, row, reads, "strided under poison")


# --------------------------------------------------------------------------------------------- the contract
def _seven(sc, slot, prm, tails=None):
    """Upload, scan and every download of the seven-read batch, the selected-rows file included."""
    sc.upload(slot, *hiplib.pack_reads(list(pc.reads())))
    if tails is not None:
        sc.set_tails(slot, tails)
    sc.scan(slot, prm)
    sc.sync()
    res = sc.results(slot).copy()
    sums, win_off = sc.window_sums(slot)
    raw, _ = sc.window_raw(slot)
    nw = np.diff(win_off)
    out = dict(results=res, win_off=win_off, sums=sums, raw=raw, read_sums=[sc.read_sums(slot, i, int(nw[i])) for i in range(len(nw))])
    if prm.flags & hiplib.F_STEP1:
        out["c_start"], out["c_end"] = sc.batch_trc_counts(slot)
    return out


def _to_fd(sc, slot, tmp_path, name, reads):
    path = str(tmp_path / name)
    fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o600)
    try:
        nbytes, crc = sc.raw_to_fd(slot, np.asarray(reads, np.int64), fd, 0)
    finally:
        os.close(fd)
    data = open(path, "rb").read()
    assert len(data) == nbytes
    return data, crc


def _check_seven(sc, slot, out, tmp_path, by_hand, tag):
    pc.assert_contract(out, by_hand=by_hand, tag=tag)
    want = pc.expected(by_hand)
    off = want["win_off"]
    for i, s in enumerate(out["read_sums"]):
        assert np.array_equal(s, want["sums"][off[i]:off[i + 1]]), (tag, "read_sums", i)
        if not want["passes"][i]:
            assert not s.any(), (tag, "read_sums of a read that does not pass", i)
    # all seven reads into a file: its bytes are window_raw's, zero rows included, and the CRC covers them
    data, crc = _to_fd(sc, slot, tmp_path, "all.bin", range(7))
    assert data == out["raw"].tobytes() == want["raw"].tobytes(), tag
    assert crc == zlib.crc32(data), tag
    # ... and a selection that starts and ends with reads that do not pass
    sel = [1, 2, 4, 5]
    data, crc = _to_fd(sc, slot, tmp_path, "sel.bin", sel)
    assert data == b"".join(want["raw"][off[i]:off[i + 1]].tobytes() for i in sel) and crc == zlib.crc32(data), tag


def test_contract_seven_reads_step1(sc, tmp_path):
    sc.set_patterns(pc.PATTERNS)
    out = twice(sc, lambda: _seven(sc, 2, pc.params()))
    _check_seven(sc, 2, out, tmp_path, False, "step 1")
    for i, seq in enumerate(pc.reads()):                # every count of every read is written, passing or not
        cs, ce = occ.trc_counts(seq, pc.PATTERNS, pc.NO_BP)
        assert out["c_start"][i].tolist() == cs and out["c_end"][i].tolist() == ce, i
    assert sc.kernel_info(2).startswith("tps_scan_kernel_s6"), sc.kernel_info(2)
    # the generic kernel (int32 sums, no padded layout) hands out the same bytes
    sc.debug_option("force_generic", 1)
    try:
        gen = twice(sc, lambda: _seven(sc, 3, pc.params()))
        assert sc.kernel_info(3).startswith("tps_scan_kernel "), sc.kernel_info(3)
    finally:
        sc.debug_option("force_generic", 0)
    _check_seven(sc, 3, gen, tmp_path, False, "step 1, generic kernel")
    _same(out, gen, "fused against generic")


def test_contract_seven_reads_tails_in_and_one_shot(sc, tmp_path):
    sc.set_patterns(pc.PATTERNS)
    out = twice(sc, lambda: _seven(sc, 2, pc.params_tails(), tails=pc.tails_in()))
    _check_seven(sc, 2, out, tmp_path, True, "TAILS_IN")
    bases, offsets = hiplib.pack_reads(list(pc.reads()))
    sums, win_off, raw = twice(sc, lambda: sc.window_counts(bases, offsets, pc.tails_in(), pc.W, pc.S, pc.T, pc.M, raw=True))
    pc.assert_contract(dict(win_off=win_off, sums=sums, raw=raw), by_hand=True, tag="window_counts")
    sums2, _, none = twice(sc, lambda: sc.window_counts(bases, offsets, pc.tails_in(), pc.W, pc.S, pc.T, pc.M, raw=False))
    assert none is None and np.array_equal(sums2, sums)


def test_contract_in_a_slot_that_held_a_larger_batch(sc, tmp_path):
    """The buffers keep their capacity and their old content: seven reads scanned where forty passing reads were, no poison."""
    sc.set_patterns(pc.PATTERNS)
    big = [pc.reads()[0] + pc.reads()[6]] * 40
    sc.upload(4, *hiplib.pack_reads(big))
    sc.scan(4, pc.params())
    sc.sync()
    res = sc.results(4)
    assert res["pass"].all() and sc.window_sums(4)[0].all() is not None and sc.window_raw(4)[0].any()
    out = _seven(sc, 4, pc.params())
    _check_seven(sc, 4, out, tmp_path, False, "after a larger batch")
    out = _seven(sc, 4, pc.params_tails(), tails=pc.tails_in())
    _check_seven(sc, 4, out, tmp_path, True, "after a larger batch, TAILS_IN")


# --------------------------------------------------------------------------------------------- wide table
# one row per planner shape (tp_cap, tw) of tests/test_gpu_wide_paths.py, the smallest read sets; one row whose tails skip a read and
# two whose filters drop reads (min_count and min_len on the anchor read's own value)
WIDE_ROWS = ["W4097_s23_m23", "W4101_s2", "W5001_s23_nobp4500", "W4501_s23_nobp6000", "nobp8000_acac_sums", "k3_W300_s7", "W4098_s23",
             "nobp8000_tails_in", "m23k21_filter_count_0", "acac16_filter_len_0"]


@pytest.mark.parametrize("rid", WIDE_ROWS)
def test_wide_rows(sc, rid):
    row = wp.BY_ID[rid]
    reads = wp.reads_of(row)
    prm = wp.params_of(row, reads)
    tails = wp.tails_of(row, reads) if prm.flags & hiplib.F_TAILS_IN else None
    out, info = twice(sc, lambda: tgwp.gpu_scan(sc, 5, row, reads, prm, tails))
    assert info.startswith(wp.WIDE + " lds="), info
    assert wp.check_scan(out, row, reads, prm, tails) > 0
    if row.filt or tails is not None:
        assert (out["results"]["pass"] == 0).any()
    # unmasked: zeros over the windows of the reads that do not pass
    skipped = np.repeat(out["results"]["pass"] == 0, np.diff(out["win_off"]))
    assert not out["sums"][skipped].any()
    if "raw" in out:
        assert not out["raw"][skipped].any()


# --------------------------------------------------------------------------------------------- every other call
def _first(cases, name_of, n, *more):
    """The first n cases plus those named in `more` (the ones with a row that contributes nothing)."""
    cases = list(cases)
    picked = cases[:n] + [c for c in cases[n:] if name_of(c) in more]
    assert {name_of(c) for c in picked} >= set(more), (more, [name_of(c) for c in cases])
    return picked


def test_followers_narrow(sc):
    """CCCTAA at k = 4 against the emulation of the kernel source and against the wide entry; reads of min_len bases or fewer and
    reads too short for a match contribute nothing."""
    import emu_driver as emu
    rng = np.random.default_rng(77)
    table = allsteps.patterns_to_search("CCCTAA", 4)
    n_fwd, follow = len(table) // 2, 2
    seqs = chk.random_reads(rng, "CCCTAA", [0, 99, 120, 150, 1999, 2000, 2001, 2500, 4200], per_base=60)
    sc.set_patterns(table)
    for lo, hi, min_len in ((100, 2000, 120), (37, 1001, 2000)):
        def call():
            sc.upload(6, *hiplib.pack_reads(seqs))
            return sc.kmer_followers(6, n_fwd, follow, lo, hi, min_len)
        picks, hist = twice(sc, call)
        want_picks, want_hist = emu.followers(table, seqs, n_fwd, follow, lo, hi, min_len)
        assert np.array_equal(picks, want_picks) and np.array_equal(hist, want_hist)
        short = [i for i, s in enumerate(seqs) if len(s) <= min_len]
        assert short and not picks[short].any() and picks.any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_followers_wide_with_and_without_histogram(sc, seed):
    from topsicle_amd import descriptive_plot as dp, seqio
    rng = np.random.default_rng(1000 + seed)
    motif, k = chk.RANDOM_SHAPES[seed % len(chk.RANDOM_SHAPES)]
    need = len(motif)
    seqs = chk.random_reads(rng, motif, [0, 99, dp.LO + need - 1, dp.LO + need, 1999, 2000, 2001, 5000])
    recs = [seqio.Record(f"r{i}", f"r{i}", s) for i, s in enumerate(seqs)]
    pats, rows, counts = twice(sc, lambda: dp.pattern_matches(recs, motif, k, 90, sc))
    want = []
    for strand in (0, 1):
        for r in recs:
            if len(r.seq) > 90:
                want += [(p, m, [r.id]) for p, m, _pos in orc.kmer_followers(r.seq, motif, k)[strand]]
    assert rows == want and len(want) > 50 and not any(ids in (["r0"], ["r1"], ["r2"]) for _p, _m, ids in want)
    table = allsteps.patterns_to_search(motif, k)
    n_fwd, follow = len(table) // 2, len(motif) - k
    sc.set_patterns_wide(table)

    def call(want_hist):
        sc.upload(6, *hiplib.pack_reads(seqs))
        return sc.kmer_followers_wide(6, n_fwd, follow, 100, 2000, 90, want_hist=want_hist)
    picks_only, none = twice(sc, lambda: call(False))
    assert none is None and picks_only.any() and not picks_only[:3].any()
    if follow <= hiplib.FOLLOW_HIST_MAX:
        picks, hist = twice(sc, lambda: call(True))
        assert np.array_equal(picks, picks_only) and int(hist.sum()) == int(np.unpackbits(picks.view(np.uint8)).sum())


def test_motif_census(sc):
    for name, reads, kw in _first(mc.cases(), lambda c: c[0], 3, "min_len", "empty"):
        def call():
            sc.upload(7, *hiplib.pack_reads(list(reads)))
            return sc.motif_census(7, want_counts=True, **kw)
        hits, counts = twice(sc, call)
        mc.assert_equal(hits, counts, name)


def test_variant_census(sc):
    for c in _first(vc.cases(), lambda c: c.name, 3, "lengths_AAAC", "empty"):
        _, unit, tails, begin, end = c.args()
        m = len(unit)
        if c.name == "lengths_AAAC":
            assert any(e - b < m for b, e in zip(begin, end)), "a tract shorter than the unit"

        def call():
            sc.upload(7, *hiplib.pack_reads(list(c.reads)))
            return sc.variant_census(7, unit, tails, begin, end, **c.kw())
        counts, profile = twice(sc, call)
        vc.assert_equal(counts, profile, c.name)


def test_tract_map(sc):
    for c in _first(tc.cases(), lambda c: c.name, 3, "ragged"):
        def call():
            sc.upload(7, *hiplib.pack_reads(list(c.reads)))
            return sc.tract_map(7, c.unit, **c.kw)
        tc.assert_equal(twice(sc, call), c.name)
    assert any(len(r) < 64 for r in tc.ragged().reads), "a read without a whole block"


def test_end_sketch_and_links(sc):
    cases = _first(ec.cases(), lambda c: c.name, 3, "bounds_k12", "letters")
    for c in cases:
        def call():
            sc.upload(7, *hiplib.pack_reads(list(c.reads)))
            return sc.end_sketch(7, c.unit, c.tails, c.begin, c.end, c.k, c.buckets)
        got = twice(sc, call)
        ec.assert_equal(got, c.name)
    assert any((np.asarray(c.end) - np.asarray(c.begin) < c.k).any() for c in cases), "an empty window"
    for name in ec.LINK_IDS[:4]:
        s, mm, ml = ec.link_sets()[name]
        got = twice(sc, lambda: sc.sketch_links(s, mm, ml))
        ec.assert_links_equal(got, ec.expected_links(name), name)
    assert "all_empty" in ec.LINK_IDS[:4], "rows that link with nothing"


def test_end_window_and_anchor_offsets(sc):
    saw_empty = saw_no_ref = False
    for c in _first(ac.cases(), lambda c: c.name, 3, "median"):
        want = ac.expected(c.name)
        codes, keep = want["codes"], want["keep"]
        if not c.by_hand:
            def call():
                sc.upload(7, *hiplib.pack_reads(list(c.reads)))
                return sc.end_window(7, c.unit, c.tails, c.begin, c.end, c.k, c.span)
            codes, keep = twice(sc, call)
            ac.assert_rows_equal((codes, keep), c.name)
            saw_empty = saw_empty or bool((np.asarray(want["length"]) < c.k).any())
        got = twice(sc, lambda: sc.anchor_offsets(codes, keep, want["length"], c.ref, c.span, c.k))
        ac.assert_offsets_equal(got, c.name)
        saw_no_ref = saw_no_ref or bool((np.asarray(c.ref) < 0).any())
    assert saw_empty and saw_no_ref, "a window shorter than k and a row without a reference"


def test_binseg_l2_and_trc_counts(sc):
    rng = np.random.default_rng(5)
    nw = [0, 1, 3, 4, 5, 9, 40, 200, 0, 777]                 # (jump 5, min_size 2: fewer than 7 windows admit no split)
    win_off = np.concatenate([[0], np.cumsum(nw)]).astype(np.int64)
    sums = np.concatenate([np.concatenate([rng.integers(40, 90, n // 2), rng.integers(0, 30, n - n // 2)]) for n in nw]).astype(np.int32)
    bkp, gain = twice(sc, lambda: sc.binseg_l2(sums, win_off, 12))
    for i, n in enumerate(nw):
        want = orc.binseg_l2_exact(sums[win_off[i]:win_off[i + 1]])
        assert bkp[i] == (-1 if want is None else want), (i, n)
    assert (bkp[[0, 1, 2, 3, 4, 8]] == -1).all() and (bkp[[6, 7, 9]] > 0).all()
    sc.set_patterns(pc.PATTERNS)
    bases, offsets = hiplib.pack_reads(list(pc.reads()))
    cs, ce = twice(sc, lambda: sc.trc_counts(bases, offsets, pc.NO_BP))
    for i, seq in enumerate(pc.reads()):
        ws, we = occ.trc_counts(seq, pc.PATTERNS, pc.NO_BP)
        assert cs[i].tolist() == ws and ce[i].tolist() == we, i
    assert not cs[3].any() and not ce[3].any() and cs.any()


# --------------------------------------------------------------------------------------------- uploads
UPLOAD_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 4097]


def _upload_reads():
    rng = np.random.default_rng(9)
    seqs = []
    for L in UPLOAD_LENGTHS:
        s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].copy()
        if L > 20:
            pos = rng.integers(0, L, max(1, L // 40))
            s[pos] = np.frombuffer(b"NnacgtRY-*", np.uint8)[rng.integers(0, 10, pos.size)]
        seqs.append(s.tobytes())
    return seqs


def _packed_equal(got, want):
    for name, g, w in zip(("seq2", "inv", "desc"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name


def test_upload_packs_like_the_host_packer(sc):
    bases, offsets = hiplib.pack_reads(_upload_reads())
    want = np_pack(bases, offsets)

    def call():
        sc.upload(8, bases, offsets)
        return sc.download_packed(8)
    _packed_equal(twice(sc, call), want)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_upload_packed(sc, pinned):
    bases, offsets = hiplib.pack_reads(_upload_reads())
    want = np_pack(bases, offsets)
    seq2, inv, desc = want
    buf = None
    if pinned:
        buf = sc.host_alloc(seq2.nbytes + inv.nbytes + desc.nbytes + 64)
        o = (seq2.nbytes + 15) & ~15
        o2 = (o + inv.nbytes + 15) & ~15
        a, b, d = buf[: seq2.nbytes].view(np.uint32), buf[o: o + inv.nbytes].view(np.uint16), buf[o2: o2 + desc.nbytes].view(hiplib.DESC_DTYPE)
        a[:], b[:], d[:] = seq2, inv, desc
        seq2, inv, desc = a, b, d

    def call():
        sc.upload_packed(8, seq2, inv, desc)
        sc.sync()
        return sc.download_packed(8)
    _packed_equal(twice(sc, call), want)
    if pinned:
        sc.host_free(buf)


def test_upload_nib4(sc):
    reads = [(s.decode().upper().translate(str.maketrans("-*", "NN")), bool(i % 2)) for i, s in enumerate(_upload_reads())]
    nib, src, desc, nw, ascii_reads = tgb._nib4_batch(reads)

    def call():
        sc.upload_nib4(8, nib, src, desc, nw)
        sc.sync()
        return sc.download_packed(8)
    got = twice(sc, call)
    assert [len(r) for r in ascii_reads] == UPLOAD_LENGTHS
    _packed_equal(got, np_pack(*hiplib.pack_reads(ascii_reads)))


# --------------------------------------------------------------------------------------------- a borrowed batch
def test_helper_with_poison_leaves_the_owners_batch_and_outputs_alone(sc):
    sc.set_patterns(pc.PATTERNS)
    reads = list(pc.reads())
    sc.upload(9, *hiplib.pack_reads(reads))
    sc.scan(9, pc.params())
    sc.sync()
    before = dict(packed=sc.download_packed(9), results=sc.results(9).copy(), sums=sc.window_sums(9), raw=sc.window_raw(9), trc=sc.batch_trc_counts(9))
    h = sc.helper(0)
    try:
        sc.debug_option("poison", 0x5A)              # (helper contexts inherit it, as they inherit the other options)
        assert h._debug.get("poison") == 0x5A
        h.set_patterns(orc.kmer_table(pc.MOTIF, 4))
        h.share(0, sc, 9)
        prm = pc.params()
        h.scan(0, prm)
        h.sync()
        mine = dict(results=h.results(0).copy(), sums=h.window_sums(0)[0], win_off=h.window_offsets(0))
        prm.slide = 12                               # a strided scan on the borrowed batch: the hidden slot borrows what is borrowed
        h.scan(0, prm)
        h.sync()
        assert "every 2nd window" in h.kernel_info(0)
    finally:
        sc.debug_option("poison", 0)
    assert mine["results"]["pass"].tolist() == pc.expected()["passes"].tolist()
    after = dict(packed=sc.download_packed(9), results=sc.results(9).copy(), sums=sc.window_sums(9), raw=sc.window_raw(9), trc=sc.batch_trc_counts(9))
    _same(before, after, "the owner's batch and outputs")
    pc.assert_contract(dict(results=after["results"], win_off=after["sums"][1], sums=after["sums"][0], raw=after["raw"][0]), tag="owner")


# --------------------------------------------------------------------------------------------- option off
def test_option_off_gives_the_same_bytes_as_under_poison(sc):
    """Runs behind the tests above (the context's buffers hold their leftovers): the default path hands out what the poisoned one did."""
    for rid in ("p_s6_filter", "sor_s6_filter", "so_s6_force_generic"):
        row = km.BY_ID[rid]
        _, batch, _ = tgkm._batches(row)
        under = twice(sc, lambda: tgkm.gpu_scan(sc, 0, row, batch))
        assert getattr(sc, "_debug", {}).get("poison") == 0
        off = tgkm.gpu_scan(sc, 0, row, batch)
        _same(under, off, rid + ": option off against poison")
    sc.set_patterns(pc.PATTERNS)
    _same(twice(sc, lambda: _seven(sc, 2, pc.params())), _seven(sc, 2, pc.params()), "seven reads: option off against poison")
