"""The oracle of tps_batch_adapter_find: the plain two-row dynamic programme on Python strings.  It shares nothing with the kernel:
no bit vectors, no packed codes, no match masks."""

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def telomere_first(read: str, tail: int) -> str:
    h = read.upper()
    return h if tail == 0 else "".join(COMP.get(c, "N") for c in reversed(h))


def find(pattern: str, text: str):
    """(dist, end): the smallest unit-cost edit distance between `pattern` and any substring text[s:e], and the smallest e that
    reaches it.  A letter of the text that is not ACGT matches nothing.  Sellers: D[0][e] = 0, D[i][0] = i."""
    m = len(pattern)
    col = list(range(m + 1))
    best, best_e = m, 0
    for e, t in enumerate(text, 1):
        new = [0] * (m + 1)
        ok = t in "ACGT"
        for i in range(1, m + 1):
            new[i] = min(col[i - 1] + (0 if ok and pattern[i - 1] == t else 1), col[i] + 1, new[i - 1] + 1)
        col = new
        if col[m] < best:
            best, best_e = col[m], e
    return best, best_e


def find_block(patterns, texts):
    """(dist, end) int arrays [n, P]: the same recurrence for every text and every pattern at once, as numpy arrays of columns
    (letters as their character codes) -- for the sets of a few hundred reads on which the plain loop above takes minutes.  The
    insertion term new[i - 1] + 1 is a running minimum of (value - i) + i.  tests/test_adapter.py holds it against find()."""
    import numpy as np
    n, P, M = len(texts), len(patterns), max(len(p) for p in patterns)
    lens = np.array([len(p) for p in patterns])
    pat = np.zeros((P, M), np.int64)
    for j, p in enumerate(patterns):
        pat[j, :len(p)] = [ord(c) for c in p]
    tlen = np.array([len(t) for t in texts])
    longest = int(tlen.max()) if n else 0
    txt = np.zeros((n, longest), np.int64)           # 0: no letter (behind the text, or not ACGT)
    for r, t in enumerate(texts):
        txt[r, :len(t)] = [ord(c) if c in "ACGT" else 0 for c in t]
    idx = np.arange(M + 1)
    col = np.tile(idx, (n, P, 1))
    best, best_e = np.tile(lens, (n, 1)), np.zeros((n, P), np.int64)
    for e in range(1, longest + 1):
        miss = (pat[None, :, :] != txt[:, e - 1, None, None]).astype(np.int64)
        a = np.zeros((n, P, M + 1), np.int64)
        a[:, :, 1:] = np.minimum(col[:, :, :-1] + miss, col[:, :, 1:] + 1)
        col = np.minimum.accumulate(a - idx, axis=2) + idx
        score = np.take_along_axis(col, np.tile(lens[None, :, None], (n, 1, 1)), axis=2)[:, :, 0]
        better = (score < best) & (tlen >= e)[:, None]
        best[better], best_e[better] = score[better], e
    return best, best_e


def adapter_find(seqs, patterns, tails, begin, end):
    """(dist, end) as lists of lists [n][P], like HipScanner.adapter_find."""
    dist, ends = [], []
    for s, t, b, e in zip(seqs, tails, begin, end):
        h = telomere_first(s, int(t))
        region = h[int(b):min(int(e), len(h))] if int(e) > int(b) else ""
        row = [find(p.upper(), region) for p in patterns]
        dist.append([r[0] for r in row])
        ends.append([r[1] for r in row])
    return dist, ends
