"""Test helper: the end sketch's and the links' rules (include/topsicle_hip.h, tps_batch_end_sketch and tps_sketch_links) and the
grouping of topsicle_amd/ends.py restated in plain Python on string slices, a set of words and lists.  Shares no code with the
product: no packed codes, no table, no staging, no ballots.  (The word set is the tract map oracle's: tests/tract_oracle.py.)"""
import numpy as np

import tract_oracle

EMPTY = 0xFFFFFFFF
_CODE = {"A": 0, "C": 1, "T": 2, "G": 3}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
M32 = 0xFFFFFFFF


def fmix32(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def telomere_first(read, tail):
    """The upper-cased read (tail 0) or its reverse complement (tail 1); a letter that is not ACGT stays one that is not (N)."""
    h = read.upper()
    return h if not tail else "".join(_COMP.get(c, "N") for c in reversed(h))


def repeat_words(unit):
    """Every word of w = min(m, 8) letters within one substitution of a cyclic word of the unit or of its reverse complement."""
    return tract_oracle.word_set(unit) | tract_oracle.word_set(tract_oracle.revcomp(unit))


def kept_positions(h, begin, end, unit, k, words=None):
    """The i in [begin, end - k] whose k-mer is kept; h is telomere first, end not yet clamped."""
    words = repeat_words(unit) if words is None else words
    w = min(len(unit), 8)
    end = min(end, len(h))
    out = []
    if end - begin < k:
        return out
    rep = [h[p:p + w] in words for p in range(begin, end - w + 1)]            # rep[p - begin]
    for i in range(begin, end - k + 1):
        if any(c not in _CODE for c in h[i:i + k]):
            continue
        if any(rep[i - begin:i - begin + k - w + 1]):
            continue
        out.append(i)
    return out


def kmer_hash(kmer):
    c = 0
    for q, ch in enumerate(kmer):
        c |= _CODE[ch] << (2 * q)
    return fmix32((c & M32) ^ 0x9E3779B9)


def sketch_read(read, tail, begin, end, unit, k, buckets, words=None):
    """(row of `buckets` hashes, kept)"""
    h = telomere_first(read, tail)
    shift = 32 - (buckets.bit_length() - 1)
    row = [EMPTY] * buckets
    kept = kept_positions(h, begin, end, unit, k, words)
    for i in kept:
        x = kmer_hash(h[i:i + k])
        row[x >> shift] = min(row[x >> shift], x)
    return row, len(kept)


def end_sketch(reads, unit, tails, begin, end, k=12, buckets=256):
    """(sketch uint32[n, buckets], kept uint32[n]) as HipScanner.end_sketch returns them."""
    words = repeat_words(unit)
    n = len(reads)
    sketch = np.full((n, buckets), EMPTY, np.uint32)
    kept = np.zeros(n, np.uint32)
    for r, read in enumerate(reads):
        sketch[r], kept[r] = sketch_read(read, int(tails[r]), int(begin[r]), int(end[r]), unit, k, buckets, words)
    return sketch, kept


def match(a, b):
    return sum(1 for x, y in zip(a, b) if x == y and x != EMPTY)


def sketch_links(sketch, min_match=6, max_links=32):
    """(degree int32[n], links int32[n, max_links], matches int32[n, max_links]) as HipScanner.sketch_links returns them.  (The
    bucket compare of one row against the rows behind it is one numpy expression: 1500 rows are a million pairs.)"""
    s = np.asarray(sketch, np.uint32)
    n = len(s)
    degree = np.zeros(n, np.int32)
    links = np.full((n, max_links), -1, np.int32)
    matches = np.zeros((n, max_links), np.int32)
    for i in range(n):
        mt = ((s[i + 1:] == s[i][None, :]) & (s[i] != EMPTY)[None, :]).sum(axis=1)
        js = [i + 1 + int(d) for d in np.nonzero(mt >= min_match)[0]]
        degree[i] = len(js)
        for p, j in enumerate(js[:max_links]):
            links[i, p], matches[i, p] = j, mt[j - i - 1]
    return degree, links, matches


def groups(n, edges, min_reads=3):
    """end[i] for i < n: connected components of the undirected `edges` [(i, j)], numbered 1, 2, ... by size, largest first, ties to
    the component whose first member comes first; 0 for the members of a component of fewer than min_reads."""
    adj = [[] for _ in range(n)]
    for i, j in edges:
        adj[i].append(j)
        adj[j].append(i)
    comp, comps = [-1] * n, []
    for s in range(n):
        if comp[s] >= 0:
            continue
        comp[s], stack, members = len(comps), [s], []
        while stack:
            v = stack.pop()
            members.append(v)
            for u in adj[v]:
                if comp[u] < 0:
                    comp[u] = comp[s]
                    stack.append(u)
        comps.append(sorted(members))
    big = sorted((c for c in comps if len(c) >= min_reads), key=lambda c: (-len(c), c[0]))
    end = [0] * n
    for g, c in enumerate(big):
        for v in c:
            end[v] = g + 1
    return end
