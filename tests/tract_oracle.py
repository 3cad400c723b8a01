"""Test helper: the tract map's rule (include/topsicle_hip.h, tps_batch_tract_map) restated in plain Python on string slices and a
set of words.  Shares no code with the product: no packed codes, no table, no staging, no state machine."""
import numpy as np

TRACT_DTYPE = np.dtype([("begin", "<i4"), ("end", "<i4"), ("hits", "<i4"), ("blocks", "<i4")])
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(u):
    return "".join(_COMP[c] for c in reversed(u))


def word_set(unit):
    """Every word of w = min(m, 8) letters within one substitution of a cyclic word of `unit`."""
    m = len(unit)
    w = min(m, 8)
    out = set()
    for j in range(m):
        word = (unit * (2 + w // m))[j:j + w]
        out.add(word)
        for q in range(w):
            for c in "ACGT":
                out.add(word[:q] + c + word[q + 1:])
    return out


def block_counts(read, words, w, block):
    """count[j] for every block of the read (none when it is shorter than w)."""
    n = len(read) - w + 1
    if n <= 0:
        return []
    hit = [read[i:i + w] in words for i in range(n)]          # (a word with an N or any other letter is in no set)
    return [sum(hit[b:b + block]) for b in range(0, n, block)]


def tracts_of(counts, L, w, block, min_hits, gap, min_blocks):
    """[(begin, end, hits, blocks)] of one strand, in order of begin."""
    flagged = [j for j, c in enumerate(counts) if c >= min_hits]
    runs = []
    for j in flagged:
        if runs and j - runs[-1][-1] <= gap + 1:
            runs[-1].append(j)
        else:
            runs.append([j])
    out = []
    for run in runs:
        b, e = run[0], run[-1] + 1
        if e - b >= min_blocks:
            out.append((b * block, min(e * block + w - 1, L), sum(counts[b:e]), e - b))
    return out


def map_read(read, unit, block=64, min_hits=20, gap=1, min_blocks=2):
    """([tracts of strand 0], [tracts of strand 1], (hits_0, hits_1, flagged_0, flagged_1))."""
    read = read.upper()
    w = min(len(unit), 8)
    per, tot = [], []
    for u in (unit, revcomp(unit)):
        counts = block_counts(read, word_set(u), w, block)
        per.append(tracts_of(counts, len(read), w, block, min_hits, gap, min_blocks))
        tot.append((sum(counts), sum(c >= min_hits for c in counts)))
    return per[0], per[1], (tot[0][0], tot[1][0], tot[0][1], tot[1][1])


def tract_map(reads, unit, block=64, min_hits=20, gap=1, min_blocks=2, max_tracts=8):
    """(tracts[n, 2, max_tracts], found int32[n, 2], totals uint32[n, 4]) as HipScanner.tract_map returns them."""
    n = len(reads)
    tracts = np.zeros((n, 2, max_tracts), TRACT_DTYPE)
    found = np.zeros((n, 2), np.int32)
    totals = np.zeros((n, 4), np.uint32)
    for r, read in enumerate(reads):
        t0, t1, tot = map_read(read, unit, block, min_hits, gap, min_blocks)
        totals[r] = tot
        for s, ts in enumerate((t0, t1)):
            found[r, s] = len(ts)
            for i, t in enumerate(ts[:max_tracts]):
                tracts[r, s, i] = t
    return tracts, found, totals
