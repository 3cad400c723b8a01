"""Test helper: the seeded case matrix of the wide-table scan (tests/test_wide_tables.py on the host emulation,
tests/test_wide_sanitizers.py on its ASan / UBSan build, tests/test_gpu_wide.py through the C ABI) and the comparison
against oracle/oracle.c, bit for bit: c_start, c_end, pass, tail, both best indices, n_win, bkp, every S_w, every raw byte.

The generators draw only inside k <= 32, P <= 64: no case is skipped or dropped."""
import numpy as np

import oracle_c
import topsicle_oracle as orc
from topsicle_amd import hiplib

MOTIFS = {16: "CTGTGGGGTCTGGGTG", 19: "ACGGATGTCACGATTCTTG", 23: "ACGGATGTCTAACTTCTTGGTGT", 25: "ACGGATTTGATTAGGTATGTGGTGT",
          26: "ACGGATTTGATTAGGTATGTGGTGTA", 32: "ACGGATGTCTAACTTCTTGGTGTACGGATTTG"}
_COMP = str.maketrans("ACGT", "TGCA")


def made_up_tables():
    """name -> pattern list: the corners a motif's own table does not reach."""
    rng = np.random.default_rng(64)
    t = {}
    seen = set()
    while len(seen) < 64:                              # P = 64 exactly: 64 distinct random 20-mers
        seen.add("".join("ACGT"[i] for i in rng.integers(0, 4, 20)))
    t["p64"] = sorted(seen)
    t["k32_allG_allA"] = ["G" * 32, "A" * 32, "C" * 32, "T" * 32, MOTIFS[32], MOTIFS[32].translate(_COMP)]
    t["homopolymer20"] = orc.kmer_table("A" * 20, 18)
    t["acac_k16"] = orc.kmer_table("AC" * 10, 16)      # every even period below k
    t["acac_k18"] = orc.kmer_table("AC" * 10, 18)
    dup = orc.kmer_table(MOTIFS[16], 14)
    t["duplicate"] = dup[:5] + [dup[2]] + dup[5:20] + [dup[2], dup[7]]
    t["narrow_ccctaa_k4"] = orc.kmer_table("CCCTAA", 4)
    return t


def motif_tables():
    """(name, motif, patterns) for every motif at k = len - 2, len, 6 and one k in 14 .. 24."""
    out = []
    for n, motif in MOTIFS.items():
        mid = {16: 14, 19: 15, 23: 21, 25: 23, 26: 24, 32: 19}[n]
        for k in sorted({n - 2, n, 6, mid}):
            out.append((f"m{n}_k{k}", motif, orc.kmer_table(motif, k)))
    return out


def _mutate(rng, s, sub=0.02, ins=0.01, dele=0.01):
    out = []
    for ch in s:
        u = rng.random()
        if u < dele:
            continue
        if u < dele + sub:
            ch = "ACGT"[rng.integers(0, 4)]
        out.append(ch)
        if rng.random() < ins:
            out.append("ACGT"[rng.integers(0, 4)])
    return "".join(out)


def make_read(rng, pats, length, kind):
    """A read with a tract the table matches at one end: repeats of a walk through the pattern list's own k-mers."""
    if length == 0:
        return ""
    body = "".join("ACGT"[i] for i in rng.integers(0, 4, length))
    k = len(pats[0])
    unit = pats[int(rng.integers(0, len(pats)))]
    tract_len = int(rng.integers(min(length, 2 * k), max(min(length, 2 * k) + 1, min(length, 2500))))
    # the unit's shortest period makes a run in which consecutive k-mers of a doubled motif all occur
    src = unit
    for other in pats:
        if other != unit and other[:-1] == unit[1:]:
            src = unit + other[-1]
            break
    tract = (src * (tract_len // len(src) + 2))[:tract_len]
    if kind != "clean":
        tract = _mutate(rng, tract)
    s = (tract + body)[:length]
    if rng.random() < 0.5:
        s = s[::-1].translate(_COMP)
    if kind == "lower":
        s = s.lower()
    elif kind == "nruns":
        b = list(s)
        for _ in range(int(rng.integers(1, 6))):
            at = int(rng.integers(0, max(1, len(b))))
            for j in range(at, min(len(b), at + int(rng.integers(1, 9)))):      # (also inside a match: the tract is where most N runs land)
                b[j] = "N" if rng.random() < 0.8 else "n"
        s = "".join(b)
    return s


def cases(n_random=300, seed=20261016, long_reads=True):
    """List of dict(name, patterns, motif_len, seqs, W, s, t, M, mode).  mode: 'sums', 'raw', 'tails' (TAILS_IN, both tails), 'step1'."""
    rng = np.random.default_rng(seed)
    tables = [(n, m, p) for n, m, p in motif_tables()] + [(n, None, p) for n, p in made_up_tables().items()]
    out = []
    modes = ["sums", "raw", "tails", "step1"]
    kinds = ["noisy", "clean", "lower", "nruns"]
    Ws, Ms, ts = [100, 60, 150, 300], [20000, 1800], [100, 0, 37]
    for ci in range(n_random):
        name, motif, pats = tables[ci % len(tables)]
        k = len(pats[0])
        mlen = len(motif) if motif else k
        slide = [mlen, 6, 7, 1, 25][(ci // len(tables) + ci) % 5]
        W = Ws[(ci // 3) % 4]
        if (W - 1) // k > 255:
            W = 100
        lens = [int(rng.integers(1200, 6000)), int(rng.integers(200, 1500)), int(rng.integers(0, k)), int(rng.integers(k, W + 1)), 0][: 2 + ci % 4]
        if slide == 1:
            lens = [min(x, 2500) for x in lens]
        seqs = [make_read(rng, pats, L, kinds[(ci + j) % 4]) for j, L in enumerate(lens)]
        out.append(dict(name=f"{ci}_{name}", patterns=pats, motif_len=mlen, seqs=seqs, W=W, s=slide, t=ts[ci % 3], M=Ms[(ci // 7) % 2], mode=modes[ci % 4]))
    if long_reads:
        for name, motif, pats in [tables[0], tables[9], tables[-1]]:          # 60 kb reads: many tiles
            seqs = [make_read(rng, pats, 60000, "noisy"), make_read(rng, pats, 60000, "nruns")]
            out.append(dict(name=f"60kb_{name}", patterns=pats, motif_len=len(pats[0]), seqs=seqs, W=100, s=6, t=100, M=60000, mode="raw"))
    return out


def params_of(c, tail_pass=None):
    base = dict(no_bp=1000, min_len=0, min_count=0, window=c["W"], slide=c["s"], trimfirst=c["t"], maxlen=c["M"])
    if c["mode"] == "step1":
        return hiplib.make_params(flags=hiplib.F_STEP1, **base)
    if c["mode"] == "tails":
        return hiplib.make_params(flags=hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_TAILS_IN | hiplib.F_STORE_SUMS | hiplib.F_STORE_RAW, **base)
    raw = hiplib.F_STORE_RAW if c["mode"] == "raw" else 0
    return hiplib.make_params(flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS | raw, **base)


def check_output(c, out, tails=None):
    """`out` = dict(results, c_start, c_end, win_off, sums, raw) of one scan of case `c` (params_of(c)); tails: what a 'tails' scan was given."""
    pats, P = c["patterns"], len(c["patterns"])
    res = out["results"]
    n_checked = 0
    for i, seq in enumerate(c["seqs"]):
        r = res[i]
        tag = (c["name"], i)
        if c["mode"] != "tails":
            cs, ce = oracle_c.trc_counts(seq, pats, 1000)
            assert out["c_start"][i].tolist() == cs, tag
            assert out["c_end"][i].tolist() == ce, tag
            assert (r["best_start"], r["best_start_idx"]) == (max(cs), cs.index(max(cs))), tag      # first maximum
            assert (r["best_end"], r["best_end_idx"]) == (max(ce), ce.index(max(ce))), tag
            tail = 0 if max(cs) > max(ce) else 1                                                     # forward only if strictly larger
            best = max(ce) if tail else max(cs)
            passed = int(len(seq) > 0 and best > 0)                                                  # min_len = 0, min_count = 0: strict
            assert r["tail"] == tail and r["pass"] == passed, tag
        else:
            tail, passed = int(tails[i]) & 1, 0 if int(tails[i]) & 2 else 1
            assert r["tail"] == tail and r["pass"] == passed, tag
        if c["mode"] == "step1" or not passed:
            assert r["n_win"] == 0 and r["bkp"] == -1, tag
            continue
        s_c, raw_c = oracle_c.window_counts(seq, "forward" if tail == 0 else "reverse", pats, c["W"], c["s"], c["t"], c["M"])
        lo, hi = int(out["win_off"][i]), int(out["win_off"][i + 1])
        assert r["n_win"] == len(s_c) == hi - lo, tag
        assert np.array_equal(out["sums"][lo:hi], s_c), tag
        if c["mode"] in ("raw", "tails"):
            assert np.array_equal(out["raw"][lo:hi], raw_c), tag
        want, _ = oracle_c.binseg_l2(s_c, P)                        # float64, numpy order: what ruptures computes
        got = int(r["bkp"])
        if r["flags"] & hiplib.RES_TIE:                             # like hiplib.resolve_ties
            got = hiplib.binseg_l2_float64(np.asarray(s_c, np.float64) / P)
        assert got == (-1 if want is None else want), tag
        n_checked += len(s_c)
    return n_checked


def tails_for(c, rng):
    """'tails' cases: both tails over the reads, and the skip bit on one of them."""
    t = rng.integers(0, 2, len(c["seqs"])).astype(np.uint8)
    if len(t) > 2:
        t[2] |= 2
    return t
