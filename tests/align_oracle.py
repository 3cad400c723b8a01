"""Test helper: the banded alignment's rule (include/topsicle_hip.h, tps_window_align) and the consensus rule of
topsicle_amd/consensus.py restated on strings with the full (n + 1) x 64 table of every pair.  Shares no code with the product: no
ballots, no direction bits, no keys -- the end cell and the path are read off the table's numbers by the rule's own words.  One
identity it does share with the kernel: the chain of "left" steps inside a row is resolved as a running minimum of D - l, which is
exact at unit cost.  The restatement that fills every cell from its three neighbours, one by one, is the stand-alone program's
(tests/emu/emu_align_main.cpp), which checks the emulation on every case of tests/align_cases.py; the emulation and the library are
both held to this oracle."""
import numpy as np

_CODE = {"A": 0, "C": 1, "T": 2, "G": 3}
LETTERS = "ACTG"
INF = 1 << 20
BAND, HALF = 64, 32
NONE, EDGE = 1, 2
DELETED, UNCOVERED = 4, 7
_LANES = np.arange(BAND, dtype=np.int64)


def pack(windows, span):
    """The codes rows tps_batch_end_window writes for these windows (a letter that is not ACGT as 0) and their lengths."""
    codes = np.zeros((len(windows), (span + 15) // 16), np.uint32)
    for r, win in enumerate(windows):
        assert len(win) <= span
        for q, ch in enumerate(win):
            codes[r, q >> 4] |= np.uint32(_CODE.get(ch, 0) << (2 * (q & 15)))
    return codes, np.array([len(w) for w in windows], np.int32)


def _codes(strings, width):
    out = np.zeros((len(strings), width), np.int64)
    for r, s in enumerate(strings):
        out[r, :len(s)] = [_CODE.get(ch, 0) for ch in s]
    return out


def tables(queries, refs, centres):
    """D[p, i, l] = D(i, i + centres[p] - 32 + l) of pair p, INF outside the matrix; the rows behind a pair's own query mean nothing.
    The pairs are walked together, row by row; the chain of "left" steps inside a row is the running minimum of D - l."""
    N = len(queries)
    n_max, m_max = max(len(q) for q in queries), max(len(r) for r in refs)
    Q, R = _codes(queries, n_max + 1), _codes(refs, m_max + 1)
    m = np.array([len(r) for r in refs], np.int64)[:, None]
    d = np.asarray(centres, np.int64)[:, None] - HALF + _LANES[None, :]
    D = np.full((N, n_max + 1, BAND), INF, np.int32)
    D[:, 0, :] = np.where((d >= 0) & (d <= m), 0, INF)
    for i in range(1, n_max + 1):
        j = i + d
        prev = D[:, i - 1, :].astype(np.int64)
        letter = np.take_along_axis(R, np.clip(j - 1, 0, m_max), axis=1)
        diag = prev + (letter != Q[:, i - 1][:, None])
        up = np.concatenate([prev[:, 1:], np.full((N, 1), INF, np.int64)], axis=1) + 1
        t = np.where((j >= 1) & (j <= m), np.minimum(np.minimum(diag, up), INF), np.where(j == 0, 0, INF))
        row = np.minimum.accumulate(t - _LANES, axis=1) + _LANES
        D[:, i, :] = np.where((j >= 0) & (j <= m), np.minimum(row, INF), INF)
    return D


def trace(T, q, r, c, span):
    """(stat[6], cols[span]) of one pair from its table T (rows of 64 numbers)."""
    n, m, d0 = len(q), len(r), c - HALF
    cols = [UNCOVERED] * span
    best = None
    for l in range(BAND):
        for i, j in {(n, n + d0 + l), (m - d0 - l, m)}:
            if 0 <= i <= n and 0 <= j <= m and T[i][l] < INF:
                key = (T[i][l], -i, -j)
                if best is None or key < best[0]:
                    best = (key, i, l)
    if best is None:
        return [0, 0, 0, 0, 0, NONE], cols
    dist, i, l = best[0][0], best[1], best[2]
    q_end, r_end = i, i + d0 + l
    j, flags, inserted = r_end, 0, []
    while i > 0 and j > 0:
        if l in (0, BAND - 1):
            flags |= EDGE
        here = T[i][l]
        s = 0 if _CODE.get(q[i - 1], 0) == _CODE.get(r[j - 1], 0) else 1
        if T[i - 1][l] < INF and here == T[i - 1][l] + s:
            move = "diagonal"
        elif l + 1 < BAND and T[i - 1][l + 1] < INF and here == T[i - 1][l + 1] + 1:
            move = "up"
        else:
            assert l > 0 and here == T[i][l - 1] + 1
            move = "left"
        if move == "up":
            inserted.insert(0, _CODE.get(q[i - 1], 0))
            i, l = i - 1, l + 1
            continue
        if inserted and j < r_end:                 # (j - 1 is covered: r_begin < j)
            cols[j] |= min(len(inserted), 3) << 3 | inserted[0] << 5 | (inserted[1] << 7 if len(inserted) >= 2 else 0)
        inserted = []
        if move == "diagonal":
            cols[j - 1] = _CODE.get(q[i - 1], 0)
            i, j = i - 1, j - 1
        else:
            cols[j - 1] = DELETED
            j, l = j - 1, l - 1
    return [dist, i, q_end, j, r_end, flags], cols


def window_align(queries, refs, ref, centre, span, pile_row=None, n_pile=0):
    """(stat int32[n, 6], cols uint16[n, span], pile int32[n_pile, span, 13] or None) as HipScanner.align_windows returns them, from the
    windows as strings."""
    n = len(queries)
    stat = np.zeros((n, 6), np.int32)
    cols = np.full((n, span), UNCOVERED, np.uint16)
    pile = np.zeros((n_pile, span, 13), np.int32) if n_pile > 0 else None
    stat[:, 5] = NONE
    have = [i for i in range(n) if ref[i] >= 0]
    if have:
        D = tables([queries[i] for i in have], [refs[ref[i]] for i in have], [centre[i] for i in have])
        for p, i in enumerate(have):
            q, r = queries[i], refs[ref[i]]
            st, cl = trace(D[p, :len(q) + 1].tolist(), q, r, int(centre[i]), span)
            stat[i], cols[i] = st, cl
            if pile is not None and pile_row is not None and pile_row[i] >= 0 and st[5] == 0:
                for j in range(st[3], st[4]):
                    v = cl[j]
                    pile[pile_row[i], j, v & 7] += 1
                    if (v >> 3) & 3:
                        pile[pile_row[i], j, 5 + ((v >> 5) & 3)] += 1
                    if ((v >> 3) & 3) >= 2:
                        pile[pile_row[i], j, 9 + ((v >> 7) & 3)] += 1
    return stat, cols, pile


def consensus(pile, R, mindepth=3):
    """The consensus of one pile row (int[span][13]) over its reference window R: None without a column of depth >= mindepth, else
    (letters, first, last, cpos) -- cpos[j] the consensus position of column j's own letter (where it would stand, for a deleted
    one), continued at one letter per column in front of `first` and behind `last`."""
    pile = np.asarray(pile)[:len(R)]
    depth = pile[:, :5].sum(axis=1)
    deep = [j for j in range(len(R)) if depth[j] >= mindepth]
    if not deep:
        return None
    first, last = deep[0], deep[-1]
    out, at = [], {}
    for j in range(first, last + 1):
        own = _CODE.get(R[j], 0)
        if depth[j] < mindepth:
            at[j] = len(out)
            out.append(own)
            continue
        ins1, ins2, states = [int(x) for x in pile[j, 5:9]], [int(x) for x in pile[j, 9:13]], [int(x) for x in pile[j, :5]]
        if 2 * sum(ins1) > depth[j]:
            out.append(ins1.index(max(ins1)))
            if 2 * sum(ins2) > depth[j]:
                out.append(ins2.index(max(ins2)))
        top = [s for s in range(5) if states[s] == max(states)]
        pick = own if own in top else top[0]
        at[j] = len(out)
        if pick != DELETED:
            out.append(pick)
    cpos = [at[first] + (j - first) if j < first else at[last] + (j - last) if j > last else at[j] for j in range(len(R))]
    return "".join(LETTERS[c] for c in out), first, last, cpos


def infix_distance(needle, hay):
    """The smallest edit distance between `needle` and any substring of `hay`."""
    b = np.frombuffer(hay.encode(), np.uint8)
    prev = np.zeros(len(b) + 1, np.int64)
    idx = np.arange(len(b) + 1, dtype=np.int64)
    for i, ch in enumerate(needle.encode(), 1):
        t = np.empty(len(b) + 1, np.int64)
        t[0] = i
        t[1:] = np.minimum(prev[:-1] + (b != ch), prev[1:] + 1)
        prev = np.minimum.accumulate(t - idx) + idx
    return int(prev.min())
