"""Test helper: the kept window's and the offset's rules (include/topsicle_hip.h, tps_batch_end_window and tps_window_offsets) and
the anchoring of topsicle_amd/anchor.py restated in plain Python on string slices, sets, dicts and sorted lists.  Shares no code with
the product: no packed k-mers, no table in an array, no histograms in bins of a wave, no ballots.  (The kept rule and the hash are
the end sketch oracle's: tests/ends_oracle.py.)"""
import numpy as np

import ends_oracle as eo

_CODE = {"A": 0, "C": 1, "T": 2, "G": 3}
EMPTY = 0xFFFFFFFF


def kept_window(read, tail, begin, end, unit, k, words=None):
    """(the window's letters, the set of window positions whose k-mer is kept)"""
    h = eo.telomere_first(read, tail)
    e = min(end, len(h))
    win = h[begin:e] if e > begin else ""
    return win, {i - begin for i in eo.kept_positions(h, begin, end, unit, k, words)}


def pack(windows, keeps, span):
    """The rows tps_batch_end_window writes for these windows: (codes uint32[n, (span + 15) // 16], keep uint32[n, (span + 31) // 32],
    length int32[n])."""
    n = len(windows)
    codes = np.zeros((n, (span + 15) // 16), np.uint32)
    keep = np.zeros((n, (span + 31) // 32), np.uint32)
    for r, (win, kp) in enumerate(zip(windows, keeps)):
        assert len(win) <= span
        for q, ch in enumerate(win):
            codes[r, q >> 4] |= np.uint32(_CODE.get(ch, 0) << (2 * (q & 15)))
        for q in kp:
            keep[r, q >> 5] |= np.uint32(1 << (q & 31))
    return codes, keep, np.array([len(w) for w in windows], np.int32)


def end_window(reads, unit, tails, begin, end, k=12, span=2000):
    """(codes, keep) as HipScanner.end_window returns them, and the windows and kept sets they were packed from."""
    words = eo.repeat_words(unit)
    wk = [kept_window(r, int(t), int(b), int(e), unit, k, words) for r, t, b, e in zip(reads, tails, begin, end)]
    windows, keeps = [w for w, _ in wk], [s for _, s in wk]
    codes, keep, _ = pack(windows, keeps, span)
    return codes, keep, windows, keeps


def table_of(win, kept, k):
    """slot -> (low 20 bits of the hash, position) of the reference: the smallest pair wins the slot."""
    t = {}
    for q in sorted(kept):
        x = eo.kmer_hash(win[q:q + k])
        cand = (x & 0xFFFFF, q)
        if (x >> 20) not in t or cand < t[x >> 20]:
            t[x >> 20] = cand
    return t


def diagonals(table, win, kept, k):
    """The sorted votes of a query against a reference's table."""
    out = []
    for p in kept:
        x = eo.kmer_hash(win[p:p + k])
        hit = table.get(x >> 20)
        if hit is not None and hit[0] == (x & 0xFFFFF):
            out.append(hit[1] - p)
    return sorted(out)


def offset_of(ds):
    """(offset, votes, second) from the sorted votes."""
    bins = {}
    for d in ds:
        bins[(d + 4096) // 64] = bins.get((d + 4096) // 64, 0) + 1
    pair = [bins.get(c, 0) + bins.get(c + 1, 0) for c in range(127)]
    best = pair.index(max(pair))
    second = max([pair[c] for c in range(127) if abs(c - best) >= 2] or [0])
    fine = [d for d in ds if 64 * best - 4096 <= d < 64 * best - 3968]
    assert len(fine) == pair[best]
    return (fine[(len(fine) - 1) // 2] if fine else 0), len(fine), second


def window_offsets(windows, keeps, ref, k=12):
    """(offset, votes, second) int32[n] as HipScanner.anchor_offsets returns them, from the windows as strings and their kept sets."""
    n = len(windows)
    out = np.zeros((3, n), np.int32)
    tables = {}
    for i in range(n):
        r = int(ref[i])
        if r < 0:
            continue
        if r not in tables:
            tables[r] = table_of(windows[r], keeps[r], k)
        out[:, i] = offset_of(diagonals(tables[r], windows[i], keeps[i], k))
    return out[0], out[1], out[2]


def lower_median(xs):
    xs = sorted(xs)
    return xs[(len(xs) - 1) // 2]


def references(end, links):
    """ref[i] for reads with group end[i] (0: none) and `links` edges each: the member with the most links, the first of them in
    run order; -1 for the ungrouped."""
    best = {}
    for i, (g, ln) in enumerate(zip(end, links)):
        if g and (g not in best or ln > links[best[g]]):
            best[g] = i
    return [best[g] if g else -1 for g in end]


def anchor(end, ref, begin, telo, offset, votes, second, min_votes=20, ratio=4):
    """Per read None (ungrouped or not anchored) or (shift, anchored length); per group its consensus position, None without an
    anchored member."""
    pos = {}
    for i, g in enumerate(end):
        if g and votes[i] >= min_votes and votes[i] >= ratio * second[i]:
            pos[i] = begin[i] + int(offset[i]) + begin[ref[i]] - begin[i]
    cons = {}
    for g in sorted(set(end) - {0}):
        mine = [pos[i] for i in pos if end[i] == g]
        cons[g] = lower_median(mine) if mine else None
    reads = [None if i not in pos else (cons[end[i]] - pos[i], telo[i] + cons[end[i]] - pos[i]) for i in range(len(end))]
    return reads, cons


def pair_errors(values, planted):
    """|(values[i] - values[j]) - (planted[i] - planted[j])| over all pairs i < j, sorted."""
    n = len(values)
    return sorted(abs((values[i] - values[j]) - (planted[i] - planted[j])) for i in range(n) for j in range(i + 1, n))

