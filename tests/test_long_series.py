"""Series of more than 3 301 windows per read (tests/long_series.py: maxlen 62 000 is 10 301 windows, 21 fused tiles) on the host:
the reads sit on the edges they claim, every row's scan through the host emulation of the kernel source equals the C oracle on a
clean and on a dirty batch, the change point takes the finish each edge read was built for (the emulation's counters), the planner
keeps its plan whatever the series' length, and the pipeline stores boundaries beyond 20 000 with --maxlengthtelo raised, the same
in one pass and in two.  The GPU half (test_gpu_long_series.py) runs the same rows and the strided batches on the MI355X.

tps_stride_kernel has no host build: the strided batches are checked here for their shape only (6 144 and 6 145 windows)."""
import csv
import os

import numpy as np
import pytest

import emu_binseg_driver as eb
import emu_driver as emu
import kernel_matrix as km
import long_series as ls
import oracle_c as occ
import test_binseg_paths as tb
import test_kernel_matrix as tkm
import test_wide_paths as twp
import topsicle_oracle as orc
import wide_path_rows as wp
from topsicle_amd import hiplib

BOUND = 1 << 31
NARROW = ls.ROWS + [ls.DEEP]


def _sums(row, seq, tail="forward"):
    sums, _ = occ.window_counts(seq, tail, row.patterns, row.W, row.s, row.t, row.M)
    return np.asarray(sums, np.int64)


def _tail_sums(row, seq):
    return _sums(row, seq, "reverse" if km.tail_of(seq, row) else "forward")


# --------------------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("row", ls.ROWS + ls.WIDE_ROWS, ids=lambda r: r.id)
def test_inputs_are_what_they_claim(row):
    clean, dirty, marks, names = ls.reads_of(row)
    assert sum(map(len, clean)) < 1 << 20 and sum(map(len, dirty)) < 1 << 20 and len(clean) <= 12
    assert all(set(x) <= set("ACGT") for x in clean)
    tw, j, ms = row.tw, row.jump, row.min_size
    n_on, n_off = ls.prefilter_edge(j, ms)
    n_M = hiplib.window_count(row.M, row.W, row.s, row.t, row.M)
    nw = [ls.nwin(row, x) for x in clean]
    assert nw[:8] == [min(x, n_M) for x in (1, 8, 7 * tw, 7 * tw + 1, 8 * tw - 1, n_on, n_off, n_M)]      # (slide 13: M holds 4 753 windows)
    assert n_off <= n_M or row.s == 13
    assert len(clean[names["two_M"]]) == 2 * row.M and len(clean[names["pure"]]) == row.M and nw[names["two_M"]] == nw[names["pure"]] == n_M
    assert n_M > 3301 and n_M > 7 * tw
    # the prefilter's edge, from binseg_from_lc's own rule: c_max - c_min < 16 x 64 candidates
    for n, on in ((n_on, True), (n_off, False)):
        c_min, c_max = ls.cand_range(n, j, ms)
        assert (c_max - c_min == ls.LCV * km.NT - (1 if on else 0)) and ls.prefilter_on(n, j, ms) == on
    assert n_off == n_on + 1 and n_off // j >= 1024
    # both strands, and every placement of the tract
    tails = [km.tail_of(x, row) for x in clean[:9]]
    assert {0, 1} <= set(tails)
    # n T >= 2^31 (the float64 D) for the dense reads, with the prefilter on for the first
    if not isinstance(row, ls.WideRow):
        for name in ("n_on", "n_off", "pure") if n_off <= n_M else ("pure",):
            s = _tail_sums(row, clean[names[name]])
            assert len(s) * int(s.sum()) >= BOUND, (name, len(s), int(s.sum()))
        s = _tail_sums(row, clean[2])
        assert len(s) == 7 * tw and len(s) * int(s.sum()) < BOUND, "the 7 tw read stays on the integer route"
    # the palindrome: more than 6 145 windows, a forward tail, S == S[::-1], and the two best exact scores equal
    if row.s <= 8:
        seq = clean[names["palindrome"]]
        s = _sums(row, seq)
        assert km.tail_of(seq, row) == 0 and len(s) > ls.STRIDE_LDS_MAX + 1 and len(s) % j == 0
        assert np.array_equal(s, s[::-1]) and s.min() < s.max()
        sc = tb.exact_scores(s, j, ms)
        assert sc[0][0] == sc[1][0] > sc[2][0] and sc[0][1] + sc[1][1] == len(s), sc[:3]
    else:
        assert "palindrome" not in names and n_M < ls.STRIDE_LDS_MAX
    # the read without a telomere and the 7 tw + 1 read (no tract) fail a filtering row's cutoff, the two shortest reads its min_len
    if getattr(row, "filt", False) is True:
        prm = row.params()
        for i, seq in enumerate(clean):
            cs, ce = occ.trc_counts(seq, row.patterns, row.no_bp)
            passes = len(seq) > prm.min_len and max(max(cs), max(ce)) > prm.min_count
            assert passes == (i not in (0, 1, 3, names["no_telomere"])), (i, len(seq))
    # the dirty copies: one letter each, where the mark says, in the coordinates of the tail step 1 picks for the copy
    tile = ls.dirty_tile(row)
    assert tile > 7 and (tile >= 14 or row.s >= 12), "past the 14th tile wherever M holds that many"
    kinds = set()
    for seq, m in zip(dirty, marks):
        if m is None:
            assert set(seq) <= set("ACGT")
            continue
        L = len(seq)
        assert [i for i, c in enumerate(seq) if c not in "ACGT"] == [m.pos], m
        assert km.tail_of(seq, row) == m.tail, m
        x = m.pos - row.t if m.tail == 0 else L - 1 - row.t - m.pos
        assert x == m.x and 0 <= x <= (ls.nwin(row, seq) - 1) * row.s + row.W - 2
        w = tile * tw + 3
        want = {f"window {w}'s first base": w * row.s, f"window {w}'s last base": w * row.s + row.W - 2,
                f"tile {tile}'s first window's first base": tile * tw * row.s, "window 3's first base": 3 * row.s}
        assert x == want[m.kind], m
        kinds.add((m.kind, m.tail))
        if m.kind == "window 3's first base":
            assert m.tail == 1 and m.pos > 65535, "the reverse tail's letter sits at a read position past 16 bits"
    assert len(kinds) == 7


def test_deep_row_has_letters_beyond_65535_of_the_scanned_string():
    clean, dirty, marks, _ = ls.deep_reads()
    row = ls.DEEP
    xs = []
    for seq, m in zip(dirty, marks):
        if m is None:
            continue
        assert [i for i, c in enumerate(seq) if c not in "ACGT"] == [m.pos] and km.tail_of(seq, row) == m.tail
        assert m.x == (m.pos - row.t if m.tail == 0 else len(seq) - 1 - row.t - m.pos)
        xs.append((m.tail, m.x))
    for tail in (0, 1):
        assert sum(1 for t, x in xs if t == tail and x > 65535) == 3, xs


def test_strided_batches_sit_on_the_lds_edge():
    """do_scan_strided keeps the compacted series in LDS up to s16_dw = 3 072 dwords per wave: max_nwin (of the batch's longest
    read, passing or not) 6 144 is the last such batch, 6 145 the first whose change point reads the series back from HBM."""
    for fam, slide, base, m in ls.STRIDED:
        row = ls.stride_row(fam, slide)
        assert slide == base * m and emu.stride_base(row.patterns, row.params(), row.M) == base
        for want, reads in zip((ls.STRIDE_LDS_MAX, ls.STRIDE_LDS_MAX + 1), ls.stride_batches(row)):
            nw = [ls.nwin(row, x) for x in reads]
            assert max(nw) == want and {0, 1, 8} <= set(nw), nw
            s16_dw = (((max(nw) + 1) // 2) + 3) & ~3
            assert (s16_dw <= 3072) == (want == ls.STRIDE_LDS_MAX)
            longest = reads[int(np.argmax(nw))]
            prm = row.params()
            best = lambda x: max(max(c) for c in occ.trc_counts(x, row.patterns, row.no_bp))
            assert best(longest) > prm.min_count and len(longest) == max(map(len, reads))
            assert sum(1 for x in reads if len(x) > prm.min_len and best(x) <= prm.min_count) == 1, "one long read does not pass"
            # the base scan's series: three and more times as many windows, beyond the 7th tile
            assert hiplib.window_count(len(longest), row.W, base, row.t, row.M) > 7 * km.Row("x", fam, s=base).tw


def test_oracle_float64_binseg_follows_numpy_beyond_one_buffer():
    """oracle.c restates ruptures' float64 Binseg with numpy's summation order; numpy sums 8 192 elements at a time.  Series whose
    answer rounding noise decides (a constant, two alternating values, a palindrome) must come out like hiplib.binseg_l2_float64,
    which runs numpy itself, on either side of 8 192 windows and far beyond."""
    rng = np.random.default_rng(3)
    for n in (8190, 8192, 8193, 10301, 16389):
        h = rng.integers(0, 97, n // 2)
        for y in (np.full(n, 94 / 12), np.tile([12, 13], n // 2 + 1)[:n] / 12, np.concatenate([h, [5] * (n % 2), h[::-1]]) / 12):
            assert occ.binseg_l2_y(y, 5, 2)[0] == hiplib.binseg_l2_float64(y, 5, 2), n


# --------------------------------------------------------------------------------------------- the rows
@pytest.mark.parametrize("row", NARROW, ids=lambda r: r.id)
def test_emulation(row):
    clean, batch = ls.batches(row)
    a = tkm.emu_scan(row, clean, dirty=False)
    n, w = km.check_scan(a, row, clean, "clean")
    b = tkm.emu_scan(row, batch, dirty=True)
    km.check_scan(b, row, batch, "dirty")
    shared = min(2, len(clean))                  # the clean batch's first reads sit in the middle of the dirty batch
    lo = (len(batch) - shared) // 2
    km.same_outputs(a, b, np.arange(shared), np.arange(lo, lo + shared), row.id + " clean reads in a dirty batch")
    if row is not ls.DEEP:
        _, _, _, names = ls.reads_of(row)
        tied = (a["results"]["flags"] & hiplib.RES_TIE) != 0
        if "palindrome" in names:
            assert tied[names["palindrome"]], "an exact tie must be flagged"
        assert w > 30000 and n == len(clean)


@pytest.mark.parametrize("row", ls.WIDE_ROWS, ids=lambda r: r.id)
def test_emulation_wide(row):
    prm = row.params()
    for reads in ls.wide_reads(row):
        out = twp.emu_scan(row, reads, prm)
        assert wp.check_scan(out, row, reads, prm) > 40000


def test_planner_keeps_the_kernel_of_the_short_series():
    for row in ls.ROWS:
        short = km.Row("x", row.family, W=row.W, s=row.s, M=20000, knobs=row.knobs, kernel=row.kernel, kernel_dirty=row.kernel_dirty)
        for dirty in (False, True):
            pl, stride = tkm._plan(row, dirty)
            ps, _ = tkm._plan(short, dirty)
            assert tkm.kernel_of_plan(row, pl) == tkm.kernel_of_plan(short, ps) == row.expected(dirty), (row.id, dirty, pl)
            assert stride == 0 and pl == ps


@pytest.mark.parametrize("fam", ["plain", "p", "r", "so", "sol", "sor", "sorh", "q", "sixteen"])
def test_plan_does_not_depend_on_the_series_length(fam):
    """The candidate sums live off-chip (lc_scratch), so variant, tw and lds_bytes are the same from 3 301 windows to the limit of
    500 000 -- and one more window is refused."""
    row = km.Row("x", fam, M=ls.M_LONG)
    emu.KNOBS.update(val_off=1, force_pair=1 if tkm._pair_kernel(km.kname(fam, 6) if fam != "sixteen" else "so") else 0)
    try:
        plans = [emu.plan_table(row.patterns, row.params(), n) for n in (3301, 10301, 66634, 500000)]
        assert all(p["variant"] == 6 for p in plans)
        assert all((p["variant"], p["tw"], p["lds_bytes"]) == (plans[0]["variant"], plans[0]["tw"], plans[0]["lds_bytes"]) for p in plans), plans
        with pytest.raises(RuntimeError, match="too many windows per read"):
            emu.plan_table(row.patterns, row.params(), 500001)
    finally:
        emu.KNOBS.update(val_off=0, force_pair=0)
    for fam_s, slide, base, _ in ls.STRIDED:
        r = km.Row("x", fam_s, s=slide)
        assert emu.stride_base(r.patterns, r.params(), 20000) == emu.stride_base(r.patterns, r.params(), 62000) == base


# --------------------------------------------------------------------------------------------- which finish ran
ROW_P = ls.BY_ID["long_p_s6"]


def _one(row, seq):
    with eb.counting() as cnt:
        out = tkm.emu_scan(row, [seq], dirty=False)
    km.check_scan(out, row, [seq], row.id)
    return out, cnt


def test_prefilter_on_with_the_float64_d():
    """5 126 windows at jump 5: 1 024 candidates, the most the prefilter holds -- and n T >= 2^31, so D goes through float64."""
    clean, _, _, names = ls.reads_of(ROW_P)
    out, cnt = _one(ROW_P, clean[names["n_on"]])
    assert cnt[eb.F64_ROUTE] == 1 and cnt[eb.ONE_LANE_FINISH] + cnt[eb.WAVE_FINISH] == 1 and cnt[eb.EXACT_TOURNAMENTS] == 0, cnt
    assert cnt[eb.ONE_LANE_FINISH] == 1 and out["results"]["bkp"][0] > 0


def test_prefilter_off_because_of_n_at_the_default_jump():
    """5 127 windows: 1 025 candidates -- no prefilter (its float64-D counter stays), every lane scores its candidates in float64."""
    clean, _, _, names = ls.reads_of(ROW_P)
    out, cnt = _one(ROW_P, clean[names["n_off"]])
    assert (cnt[eb.F64_ROUTE], cnt[eb.ONE_LANE_FINISH], cnt[eb.WAVE_FINISH], cnt[eb.CROWDED], cnt[eb.EXACT_TOURNAMENTS]) == (0, 0, 1, 0, 0), cnt
    assert out["results"]["bkp"][0] > 0
    out, cnt = _one(ROW_P, clean[names["at_M"]])
    assert (cnt[eb.F64_ROUTE], cnt[eb.ONE_LANE_FINISH], cnt[eb.WAVE_FINISH]) == (0, 0, 1), cnt


def test_integer_route_and_one_lane_finish_beyond_the_seventh_tile():
    clean, _, _, _ = ls.reads_of(ROW_P)
    out, cnt = _one(ROW_P, clean[3])                 # 7 tw + 1 windows, no tract: the first window of tile 7
    assert cnt[eb.F64_ROUTE] == 0 and cnt[eb.ONE_LANE_FINISH] + cnt[eb.WAVE_FINISH] == 1, cnt
    out, cnt = _one(ROW_P, clean[2])
    assert cnt[eb.F64_ROUTE] == 0 and cnt[eb.ONE_LANE_FINISH] + cnt[eb.WAVE_FINISH] == 1, cnt


@pytest.mark.parametrize("rid", ["long_p_s6", "long_so_s6", "long_sorh_s6"])
def test_exact_tournament_on_a_series_of_more_than_6145_windows(rid):
    row = ls.BY_ID[rid]
    clean, _, _, names = ls.reads_of(row)
    out, cnt = _one(row, clean[names["palindrome"]])
    assert out["results"]["n_win"][0] > 6145 and cnt[eb.EXACT_TOURNAMENTS] == 1, cnt
    assert out["results"]["flags"][0] & hiplib.RES_TIE
    assert out["results"]["bkp"][0] > out["results"]["n_win"][0] // 2, "the later of the two mirrored splits"


# --------------------------------------------------------------------------------------------- the pipeline
PIPE_SEED = 7
PIPE_M = 45000


def pipeline_reads(seed=PIPE_SEED):
    """[(id, sequence)]: twelve reads with tracts of 22 000 to 40 000 bases on either strand (ONT-like errors), then short,
    non-telomeric and very long ones."""
    rng = np.random.default_rng([seed, 0x7E10])
    out = []
    for i in range(12):
        tract = int(rng.integers(22000, 40001))
        L = tract + int(rng.integers(3000, 12000))
        seq = km._tract("CCCTAA", tract, rng, err=0.02) + km._rand(L - tract, rng)
        out.append((f"telo{i}", seq if i % 2 == 0 else seq[::-1].translate(km.COMP)))
    for i, L in enumerate((1500, 8000, 9001, 12000)):
        a = min(L // 3, 2500)
        out.append((f"short{i}", km._tract("CCCTAA", a, rng, err=0.02) + km._rand(L - a, rng)))
    for i, L in enumerate((11000, 30000, 47000, 52000)):
        out.append((f"none{i}", km._rand(L, rng)))
    for i, (L, tract) in enumerate(((46000, 5000), (60000, 30000), (90000, 44000), (50000, 46000))):
        seq = km._tract("CCCTAA", tract, rng, err=0.02) + km._rand(L - tract, rng)
        out.append((f"long{i}", seq if i % 2 else seq[::-1].translate(km.COMP)))
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def write_fasta(path, recs):
    with open(path, "w") as h:
        for rid, s in recs:
            h.write(f">{rid}\n" + "\n".join(s[j:j + 80] for j in range(0, len(s), 80)) + "\n")


_lengths: dict = {}


def oracle_lengths(recs, maxlen, cutoff=0.7, min_len=9000):
    """{id: telo_length} of the reads the oracle's step 1 keeps (k = 4, the CLI's defaults).  Computed once per maxlen and shared."""
    if maxlen not in _lengths:
        _lengths[maxlen] = _oracle_lengths(recs, maxlen, cutoff, min_len)
    return dict(_lengths[maxlen])


def _oracle_lengths(recs, maxlen, cutoff, min_len):
    pats = orc.kmer_table("CCCTAA", 4)
    out = {}
    for rid, seq in recs:
        if len(seq) <= min_len:
            continue
        cs, ce = orc.trc_counts(seq, pats)
        call = orc.trc_call(cs, ce, pats, 6, cutoff)
        if call:
            out[rid] = orc.step2(seq, call[1], pats, 100, 6, 100, maxlen)
    return out


def run_cli(run, recs, root, extra):
    """One run of the CLI on `recs`: ({id: telo_length}, normalised outputs)."""
    import cli_cases
    os.makedirs(root, exist_ok=True)
    fa = os.path.join(root, "reads.fasta")
    write_fasta(fa, recs)
    out = os.path.join(root, "out")
    os.makedirs(out, exist_ok=True)
    assert run(["-i", fa, "-o", out, "--pattern", "CCCTAA", "--threads", "1"] + extra) in (None, 0)
    rows = list(csv.reader(open(os.path.join(out, "telolengths_all.csv"))))
    got = {r[3]: int(r[4]) for r in rows[1:]}
    assert len(got) == len(rows) - 1
    return got, cli_cases.normalise(out)


def check_pipeline(run, tmp_path):
    recs = pipeline_reads()
    assert len(recs) == 24
    want = oracle_lengths(recs, PIPE_M)
    assert sum(1 for v in want.values() if v > 20000) >= 8 and max(want.values()) <= PIPE_M
    runs = {}
    for mode in ("off", "on"):
        got, norm = run_cli(run, recs, str(tmp_path / mode), ["--maxlengthtelo", str(PIPE_M), "--twopass", mode])
        assert got == want, (mode, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)})
        runs[mode] = norm
    assert runs["off"] == runs["on"]
    got, _ = run_cli(run, recs, str(tmp_path / "default"), [])
    assert got == oracle_lengths(recs, 20000) and set(got) == set(want) and max(got.values()) <= 20000


def test_oracle_puts_the_pipeline_reads_where_they_claim():
    recs = pipeline_reads()
    want = oracle_lengths(recs, PIPE_M)
    assert {f"telo{i}" for i in range(12)} <= set(want) and not any(k.startswith(("none", "short0", "short1")) for k in want)
    assert sum(1 for v in want.values() if v > 20000) >= 8
    assert max(oracle_lengths(recs, 20000).values()) <= 20000


def test_pipeline_stores_boundaries_beyond_20000(tmp_path, emu_engine_factory):
    from test_ref_cli_differential import run_product
    check_pipeline(lambda argv: run_product(emu_engine_factory(), argv), tmp_path)
