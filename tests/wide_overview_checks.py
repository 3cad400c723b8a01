"""Test helper: the checks of the k-mer / follower counts on wide tables (tps_batch_kmer_followers_wide), shared by
tests/test_wide_overview.py (the kernel source through the emulation) and tests/test_gpu_wide_overview.py (the kernel through
the C ABI).  `engine` is anything with HipScanner's interface."""
import json
import os

import numpy as np

import record_wide_overview as rec
import topsicle_oracle as orc
from topsicle_amd import allsteps, descriptive_plot as dp, hiplib, seqio

M15 = rec.M16[:15]
# (motif, k) of the random-read check: the recorded shapes and a 15-letter motif whose k = 6 leaves 9 letters to follow
RANDOM_SHAPES = [(rec.M16, 14), (rec.M23, 21), (rec.M32, 30), (rec.M23, 6), (rec.M32, 4), (rec.M16, 4), (M15, 6)]
E2E_MOTIFS = {"m16": rec.M16, "m23": rec.M23, "m32": rec.M32}


def fixture_records(name, gold_dir, tmp_dir):
    """(fixture, records) of tests/golden/wideov_<name>.json: the seeded input rebuilt, checked against the recorded digest, read
    by the product's own reader."""
    import cli_cases
    fx = json.load(open(os.path.join(gold_dir, f"wideov_{name}.json")))
    case = rec.make_case(name)
    assert cli_cases.case_digest(case) == fx["case_sha256"], "the seeded input no longer is what the fixture was recorded from"
    inp, _out = cli_cases.materialise(case, str(tmp_dir))
    return fx, list(seqio.read_records(inp))


def check_fixture(name, gold_dir, tmp_dir, engine):
    """Row sequence, digest and crosstab of one recorded run of the reference."""
    fx, recs = fixture_records(name, gold_dir, tmp_dir)
    pats, rows, counts = dp.pattern_matches(recs, fx["motif"], fx["k"], fx["minSeqLength"], engine)
    print(f"{name}: {len(rows)} rows (recorded {fx['n_rows']})")
    assert len(rows) == fx["n_rows"]
    assert [[r[0], r[1], r[2]] for r in rows[:25]] == fx["first_rows"]
    assert rec.rows_digest(rows) == fx["rows_sha256"]
    # rows of the reads come first, then those of the reverse complements: the boundary is where the recorded count says
    n0 = fx["rows_per_strand"][0]
    want0 = sum(len(orc.kmer_followers(r.seq, fx["motif"], fx["k"])[0]) for r in recs if len(r.seq) > fx["minSeqLength"])
    assert n0 == want0 and fx["rows_per_strand"][1] == len(rows) - n0
    follow = len(fx["motif"]) - fx["k"]
    if follow > rec.HIST_MAX_FOLLOW:
        assert counts is None and "counts" not in fx
        return
    patterns, matches, tab = rec.crosstab(rows)
    assert patterns == fx["patterns"] and matches == fx["matches"] and tab == fx["counts"]
    # the device-side crosstab: same numbers, bins in 2-bit code order (+ one bin for non-ACGT followers)
    labels = dp.follower_labels(follow)
    assert counts.shape == (len(pats), 4 ** follow + 1) and int(counts.sum()) == fx["n_rows"]
    for j, p in enumerate(pats):
        for b, lab in enumerate(labels):
            want = fx["counts"][fx["matches"].index(lab)][fx["patterns"].index(p)] if lab in fx["matches"] and p in fx["patterns"] else 0
            assert counts[j, b] == want, (p, lab)


def random_reads(rng, motif, lengths, per_base=150):
    """Reads of the given lengths: a tract of the motif from a random phase, random bases behind it, one base in `per_base`
    replaced by a letter of "ACGTNacgtnR", as they are or reverse-complemented."""
    seqs = []
    for L in lengths:
        tract = int(rng.integers(0, max(1, L)))
        ph = int(rng.integers(len(motif)))
        body = list(((motif * (tract // len(motif) + 2))[ph:ph + tract] + "".join("ACGT"[x] for x in rng.integers(0, 4, max(0, L - tract))))[:L])
        for p in rng.integers(0, max(1, L), L // per_base):
            if body:
                body[p] = "ACGTNacgtnR"[int(rng.integers(11))]
        s = "".join(body)
        if L >= 1999 and rng.random() < 0.5:
            s = s[:300] + s[300:700].lower() + s[700:]
        seqs.append(s if rng.random() < 0.5 else s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca")))
    return seqs


def check_random_reads_against_oracle(engine, seed):
    """tests/test_overview_plot.py's random-read check on long motifs and long followers, against oracle.kmer_followers."""
    rng = np.random.default_rng(1000 + seed)
    motif, k = RANDOM_SHAPES[seed % len(RANDOM_SHAPES)]
    need = len(motif)                                  # k + follow
    lengths = [0, 99, dp.LO + need - 1, dp.LO + need, 1999, 2000, 2001, 5000, 1999, 2500, 5000, 9000]
    seqs = random_reads(rng, motif, lengths)
    # the shortest read that can hold a match holds one: the motif right at base LO
    seqs[3] = "".join("ACGT"[x] for x in rng.integers(0, 4, dp.LO)) + (motif * 2)[:need]
    recs = [seqio.Record(f"r{i}", f"r{i}", s) for i, s in enumerate(seqs)]
    min_len = 90
    pats, rows, counts = dp.pattern_matches(recs, motif, k, min_len, engine)
    want = []
    for strand in (0, 1):
        for r in recs:
            if len(r.seq) > min_len:
                want += [(p, m, [r.id]) for p, m, _pos in orc.kmer_followers(r.seq, motif, k)[strand]]
    print(f"{motif} k={k}: {len(rows)} rows (oracle {len(want)})")
    assert rows == want
    assert len(want) > 200 and any(ids == ["r3"] for _p, _m, ids in want) and not any(ids == ["r2"] for _p, _m, ids in want)
    follow = len(motif) - k
    if follow > hiplib.FOLLOW_HIST_MAX:
        assert counts is None
        return
    labels = dp.follower_labels(follow)
    for j, p in enumerate(pats):
        mine = [m for q, m, _ in want if q == p]
        for b, lab in enumerate(labels):
            assert counts[j, b] == mine.count(lab)
        assert counts[j, -1] == sum(1 for m in mine if set(m) - set("ACGT"))


def check_old_against_new(engine, seed=0):
    """On a table both entries accept, picks and histogram are the same bits: CCCTAA at k = 4, a 15-letter motif at k = 13."""
    rng = np.random.default_rng(77 + seed)
    for motif, k in (("CCCTAA", 4), (M15, 13)):
        table = allsteps.patterns_to_search(motif, k)
        n_fwd, follow = len(table) // 2, len(motif) - k
        seqs = random_reads(rng, motif, [0, 99, 150, 1999, 2000, 2001, 2500, 5000, 9000, 4200], per_base=60)
        bases, offsets = hiplib.pack_reads(seqs)
        for lo, hi, min_len in ((100, 2000, 120), (0, 4096, 0), (37, 1001, 2000)):
            engine.set_patterns(table)
            engine.upload(0, bases, offsets)
            picks_n, hist_n = engine.kmer_followers(0, n_fwd, follow, lo, hi, min_len)
            engine.set_patterns_wide(table)
            picks_w, hist_w = engine.kmer_followers_wide(0, n_fwd, follow, lo, hi, min_len)
            print(f"{motif} k={k} [{lo}, {hi}): {int(hist_n.sum())} picks")
            assert picks_n.shape == picks_w.shape and np.array_equal(picks_n, picks_w)
            assert np.array_equal(hist_n, hist_w) and int(hist_n.sum()) == int(np.unpackbits(picks_w.view(np.uint8)).sum())
            picks_only, none = engine.kmer_followers_wide(0, n_fwd, follow, lo, hi, min_len, want_hist=False)
            assert none is None and np.array_equal(picks_only, picks_w)
        assert int(hist_n.sum()) > 0


def check_error_paths(engine):
    """What tps_batch_kmer_followers_wide refuses, and what keeps being refused elsewhere."""
    import pytest
    wide = allsteps.patterns_to_search(rec.M23, 21)                # 46 patterns of 21 letters
    narrow = allsteps.patterns_to_search("CCCTAA", 4)
    bases, offsets = hiplib.pack_reads(["ACGT" * 700, rec.M23 * 100])
    engine.set_patterns_wide(wide)
    engine.upload(0, bases, offsets)
    picks, hist = engine.kmer_followers_wide(0, 23, 2)             # the legal call
    assert picks.shape == (2, 2, 23, 60) and hist.shape == (2, 23, 17) and hist.sum() > 0
    for kw in (dict(n_fwd=0, follow=2), dict(n_fwd=33, follow=2), dict(n_fwd=24, follow=2),            # 2 n_fwd > P
               dict(n_fwd=23, follow=-1), dict(n_fwd=23, follow=2, lo=0, hi=4097), dict(n_fwd=23, follow=2, lo=500, hi=500),
               dict(n_fwd=23, follow=9, want_hist=True)):
        with pytest.raises(hiplib.TopsicleHipError):
            engine.kmer_followers_wide(0, **kw)
    picks, hist = engine.kmer_followers_wide(0, 23, 9, want_hist=False)       # nine followers without the histogram: fine
    assert hist is None and picks.any()
    picks, hist = engine.kmer_followers_wide(0, 23, 2, 0, 4096)                # the whole span
    assert picks.shape == (2, 2, 23, 128)
    with pytest.raises(hiplib.TopsicleHipError):                   # the narrow entry keeps refusing a wide table
        engine.kmer_followers(0, 15, 2)
    engine.set_patterns(narrow)
    with pytest.raises(hiplib.TopsicleHipError):                   # ... and the wide entry wants a table of set_patterns_wide
        engine.kmer_followers_wide(0, 6, 2)
    engine.set_patterns_wide(narrow)                               # (which takes narrow tables too)
    assert engine.kmer_followers_wide(0, 6, 2)[0].shape == (2, 2, 6, 60)
    recs = [seqio.Record("r0", "r0", "ACGT" * 700)]
    with pytest.raises(hiplib.TopsicleHipError, match="up to 32 letters"):     # one clear error beyond 32 letters
        dp.pattern_matches(recs, rec.M32 + "A", 31, 120, engine)


def e2e_reads(motif, seed):
    """Ten reads of 3000 bases for the overview driver: a tract of 2200 bases with at most 0.5 % substitutions and random bases
    behind it, every other one reverse-complemented; reads 3 and 7 hold no tract.  Returns [(id, seq)]."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(10):
        ph = int(rng.integers(len(motif)))
        tract = list((motif * (2200 // len(motif) + 2))[ph:ph + 2200]) if i not in (3, 7) else []
        for p in rng.choice(len(tract), int(rng.integers(0, 12)), replace=False) if tract else []:       # <= 11 of 2200: 0.5 %
            tract[p] = "ACGT"[int(rng.integers(4))]
        s = "".join(tract) + "".join("ACGT"[x] for x in rng.integers(0, 4, 3000 - len(tract)))
        out.append((f"e{seed}_{i}", s if i % 2 == 0 else s[::-1].translate(str.maketrans("ACGT", "TGCA"))))
    return out


def check_overview_end_to_end(tmp_path, motif, engines):
    """overview_plot --recfindingpattern --rawcount on a generated FASTQ: the reads the oracle's step 1 lets through at the
    upstream cutoff of 0.7, and for them the CSV's rows == the oracle's.  engines=None: the driver opens the GPU itself."""
    import pandas as pd
    from topsicle_amd import overview_plot
    k, min_len = len(motif) - 2, 1200
    reads = e2e_reads(motif, 4242 + len(motif))
    fq = tmp_path / "reads.fastq"
    fq.write_text("".join(f"@{rid}\n{s}\n+\n{'I' * len(s)}\n" for rid, s in reads))
    pats = orc.kmer_table(motif, k)
    passing = []
    for rid, s in reads:
        cs, ce = orc.trc_counts(s, pats)
        if len(s) > min_len and orc.trc_call(cs, ce, pats, len(motif), overview_plot.TRC_CUTOFF) is not None:
            passing.append((rid, s))
    print(f"{motif}: {len(passing)} of {len(reads)} reads pass the oracle's step 1")
    assert len(passing) >= 6
    want = []
    for strand in (0, 1):
        for rid, s in passing:
            want += [(p, m, rid) for p, m, _pos in orc.kmer_followers(s, motif, k)[strand]]
    out = tmp_path / "ov"
    argv = ["--inputDir", str(fq), "--outputDir", str(out), "--pattern", motif, "--minSeqLength", str(min_len), "--recfindingpattern", "--rawcount"]
    if engines is None:
        overview_plot.main(argv)
    else:
        overview_plot.run(overview_plot.build_parser().parse_args(argv), engines=engines)
    assert (out / "descriptive_plot_1.png").stat().st_size > 1000 and (out / "heatmap_1.png").stat().st_size > 1000
    df = pd.read_csv(out / "heatmap_rawcount_1.csv", keep_default_na=False)
    assert list(df.columns) == ["Pattern", "Match", "read id"]
    got = [(p, m, i.strip("[]'")) for p, m, i in df.values.tolist()]
    print(f"{len(got)} rows in the CSV (oracle {len(want)})")
    assert got == want and len(want) > 1000
