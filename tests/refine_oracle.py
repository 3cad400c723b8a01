"""Test helper: the rule of tps_batch_boundary_refine (include/topsicle_hip.h) restated in plain Python on strings, prefix sums in a
list.  Shares no code with the product: no packed codes, no table, no staging, no ballots."""
import numpy as np

REFINE_DTYPE = np.dtype([(f, "<i4") for f in ("pos", "score", "drop", "at_score", "hits_before", "hits_after", "runner", "runner_pos")])
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def telomere_first(read, tail):
    """The upper-cased read (tail 0) or its reverse complement (tail 1); a letter that is not ACGT stays one that is not."""
    h = read.upper()
    return h if tail == 0 else "".join(_COMP.get(c, "N") for c in reversed(h))


def word_set(unit):
    """Every word of w = min(m, 8) letters within one substitution of a cyclic word of `unit`."""
    m = len(unit)
    w = min(m, 8)
    out = set()
    for j in range(m):
        word = (unit * (2 + w // m))[j:j + w]
        for q in range(w):
            for c in "ACGT":
                out.add(word[:q] + c + word[q + 1:])
    return out


def hits(h, unit, begin, end):
    """x_i for i in [begin, begin + N): a word with any other letter is in no set."""
    w = min(len(unit), 8)
    words = word_set(unit)
    n = min(end, len(h)) - begin - w + 1
    return [1 if h[i:i + w] in words else 0 for i in range(begin, begin + max(n, 0))]


def refine_hits(x, begin, at, hit=2, miss=1, sep=200):
    """The row of one read from its hits x (a list of 0 / 1), as a tuple in the order of REFINE_DTYPE."""
    n = len(x)
    if n == 0:
        return (begin, 0, 0, 0, 0, 0, 0, -1)
    P = [0]
    for v in x:
        P.append(P[-1] + (hit if v else -miss))
    score = max(P)
    rel = P.index(score)                            # the smallest
    far = [j for j in range(n + 1) if abs(j - rel) >= sep]
    runner, runner_pos = 0, -1
    if far:
        runner = max(P[j] for j in far)
        runner_pos = begin + min(j for j in far if P[j] == runner)
    before = sum(x[:rel])
    return (begin + rel, score, score - P[n], P[min(max(at, begin), begin + n) - begin], before, sum(x) - before, runner, runner_pos)


def refine_read(read, unit, tail, begin, end, at, hit=2, miss=1, sep=200):
    return refine_hits(hits(telomere_first(read, tail), unit, begin, end), begin, at, hit, miss, sep)


def boundary_refine(reads, unit, tails, begin, end, at, hit=2, miss=1, sep=200):
    """REFINE_DTYPE[n] as HipScanner.boundary_refine returns it."""
    out = np.zeros(len(reads), REFINE_DTYPE)
    for r, read in enumerate(reads):
        out[r] = refine_read(read, unit, int(tails[r]), int(begin[r]), int(end[r]), int(at[r]), hit, miss, sep)
    return out
