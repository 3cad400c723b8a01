"""The seven-read batch on which the contract for reads that do not pass is stated (include/topsicle_hip.h, "Reads that do not
pass"), shared by tests/test_poison_contract.py (the host emulation) and tests/test_gpu_poison.py (the MI355X).  Not collected by
pytest: no test_ prefix.

One table (CCCTAA, k = 5), window 100, slide 6, trimfirst 100, min_len 1000, the 0.4 cutoff's min_count, sums and raw rows stored.
The reads, in order: passing; 900 bases of tract (too short, with windows in the layout); 3000 random bases (below the cutoff);
empty; passing with an N; 1001 random bases (long enough, below the cutoff); passing on the reverse tail.  `expected()` is the
whole answer from oracle/oracle.c: pass and tail per read, the window layout, and S_w and raw rows with ZEROS over exactly the
ranges of the reads that do not pass -- for the step-1 scan, and for a scan whose tails come from the caller (TAILS, bit 1 = skip
on reads 1 and 4), which is also what the one-shot window_counts call must return."""
import functools

import numpy as np

import oracle_c as occ
import topsicle_oracle as orc
from topsicle_amd import allsteps, hiplib

MOTIF, K = "CCCTAA", 5
W, S, T, M, NO_BP, MIN_LEN, CUTOFF = 100, 6, 100, 20000, 1000, 1000, 0.4
FLAGS = hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS | hiplib.F_STORE_RAW
FLAGS_TAILS = hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_TAILS_IN | hiplib.F_STORE_SUMS | hiplib.F_STORE_RAW
PATTERNS = orc.kmer_table(MOTIF, K)
P = len(PATTERNS)
MIN_COUNT = allsteps.min_count_for_cutoff(CUTOFF, NO_BP / len(MOTIF), NO_BP)
SKIP_BY_HAND = (1, 4)         # the reads whose tails carry bit 1 in the TAILS_IN scan
_COMP = str.maketrans("ACGT", "TGCA")


@functools.lru_cache(maxsize=None)
def reads():
    rng = np.random.default_rng(20261019)
    rand = lambda n: "".join("ACGT"[x] for x in rng.integers(0, 4, n))      # noqa: E731
    tract = lambda n: (MOTIF * (n // len(MOTIF) + 1))[:n]                   # noqa: E731
    with_n = tract(700) + rand(520)
    with_n = with_n[:350] + "N" + with_n[351:]
    return (tract(800) + rand(306), tract(900), rand(3000), "", with_n, rand(1001), (tract(640) + rand(700))[::-1].translate(_COMP))


def params():
    return hiplib.make_params(no_bp=NO_BP, min_len=MIN_LEN, min_count=MIN_COUNT, window=W, slide=S, trimfirst=T, maxlen=M, flags=FLAGS)


def params_tails():
    return hiplib.make_params(no_bp=NO_BP, min_len=0, min_count=-1, window=W, slide=S, trimfirst=T, maxlen=M, flags=FLAGS_TAILS)


@functools.lru_cache(maxsize=None)
def _step1():
    """(tail, pass) per read as oracle.c's step 1 decides: forward only if strictly larger; both filters are strict."""
    tail, ok = [], []
    for seq in reads():
        cs, ce = occ.trc_counts(seq, PATTERNS, NO_BP)
        t = 0 if max(cs) > max(ce) else 1
        tail.append(t)
        ok.append(int(len(seq) > MIN_LEN and (max(ce) if t else max(cs)) > MIN_COUNT))
    return np.array(tail, np.int32), np.array(ok, np.int32)


def tails_in():
    """What the TAILS_IN scan and window_counts are handed: step 1's tails, bit 1 (skip) on SKIP_BY_HAND."""
    t = _step1()[0].astype(np.uint8)
    t[list(SKIP_BY_HAND)] |= 2
    return t


@functools.lru_cache(maxsize=None)
def expected(by_hand=False):
    """dict(tail, pass, win_off, sums, raw, skipped): the oracle's windows for the reads that pass, zeros for the others."""
    tail, ok = _step1()
    if by_hand:
        ok = np.array([0 if i in SKIP_BY_HAND else 1 for i in range(len(reads()))], np.int32)
    nw = np.array([hiplib.window_count(len(x), W, S, T, M) for x in reads()], np.int64)
    win_off = np.concatenate([[0], np.cumsum(nw)])
    sums = np.zeros(int(win_off[-1]), np.int32)
    raw = np.zeros((int(win_off[-1]), P), np.uint8)
    for i, seq in enumerate(reads()):
        if ok[i] and nw[i]:
            s, r = occ.window_counts(seq, "reverse" if tail[i] else "forward", PATTERNS, W, S, T, M)
            sums[win_off[i]:win_off[i + 1]] = s
            raw[win_off[i]:win_off[i + 1]] = r
    skipped = np.zeros(int(win_off[-1]), bool)
    for i in np.nonzero(ok == 0)[0]:
        skipped[win_off[i]:win_off[i + 1]] = True
    for a in (tail, ok, win_off, sums, raw, skipped):
        a.setflags(write=False)
    return dict(tail=tail, passes=ok, win_off=win_off, sums=sums, raw=raw, skipped=skipped)


def assert_contract(out, by_hand=False, tag=""):
    """`out` = dict(results, win_off, sums, raw) of one scan of reads() (no results: the one-shot window_counts call): pass against
    the oracle, zeros over exactly the ranges of the reads that do not pass, the oracle's windows everywhere else."""
    want = expected(by_hand)
    res = out.get("results")
    assert 0 < want["passes"].sum() < len(want["passes"])                 # neither all 0 nor all 1
    if res is not None:
        assert np.array_equal(res["pass"], want["passes"]), (tag, res["pass"].tolist(), want["passes"].tolist())
        assert np.array_equal(res["tail"], want["tail"]), tag
    assert np.array_equal(out["win_off"], want["win_off"]), tag
    off, skipped = want["win_off"], want["skipped"]
    assert skipped.any() and not skipped.all()
    sums, raw = np.asarray(out["sums"]), np.asarray(out["raw"]).reshape(-1, P)
    assert sums.shape == want["sums"].shape and raw.shape == want["raw"].shape, tag
    assert not sums[skipped].any(), (tag, "S_w of the reads that do not pass", np.nonzero(sums[skipped])[0][:8].tolist())
    assert not raw[skipped].any(), (tag, "raw rows of the reads that do not pass")
    for i in np.nonzero(want["passes"])[0]:
        lo, hi = off[i], off[i + 1]
        bad = np.nonzero(sums[lo:hi] != want["sums"][lo:hi])[0]
        assert not len(bad), (tag, f"read {i}: S_w differs first at window {bad[0]}: got {sums[lo + bad[0]]}, oracle {want['sums'][lo + bad[0]]}")
        badr = np.argwhere(raw[lo:hi] != want["raw"][lo:hi])
        assert not len(badr), (tag, f"read {i}: raw row differs first at window {badr[0][0]} pattern {badr[0][1]}")
        assert res is None or res["n_win"][i] == hi - lo, (tag, int(i))
    # (the windows of the passing reads are not all zero: the zeros above are the contract's, not an empty answer)
    assert sums[~skipped].any() and raw[~skipped].any(), tag
    for i in np.nonzero(want["passes"] == 0)[0]:
        assert res is None or (res["n_win"][i] == 0 and res["bkp"][i] == -1), (tag, int(i))
