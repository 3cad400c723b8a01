"""Test helper: the motif census restated from its definition (include/topsicle_hip.h, tps_batch_motif_census) in plain
Python / NumPy, one read end and one period at a time -- no bit planes, no words, no lanes: nothing of the kernel's text.

For a read of length L and an end e, h = bases [lo, min(L, hi)) of the upper-cased read (e = 0) or of its reverse complement
(e = 1), n = len(h).  For a period u, w = min(u, 8):
    eq_u[i]  = i + u < n, h[i] and h[i + u] both one of ACGT, and equal
    per_u[i] = i + u + w <= n and eq_u[i .. i + w - 1] all set
    C_u      = sum(per_u)
u* = arg max C_u (ties: the smallest u); the run = the longest maximal run of per_u* (ties: the leftmost); unit = h[run_start ..
run_start + u*) as 2-bit codes A C T G = 0 1 2 3, letter j in bits [2j, 2j+1].  All zeros where no C_u is positive and for reads with
L <= min_len."""
import numpy as np

from topsicle_amd import hiplib

W_CAP = 8
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
_CODE = {"A": 0, "C": 1, "T": 2, "G": 3}


def end_string(seq: str, e: int, lo: int, hi: int) -> str:
    s = seq.upper()
    if e == 1:
        # reverse complement; a letter that is not ACGT stays what it is (it equals nothing either way)
        s = s.encode("ascii", "replace").translate(_COMP)[::-1].decode("ascii")
    return s[lo:min(len(s), hi)]


def per_bits(h: str, u: int) -> np.ndarray:
    """per_u as a bool array of len(h) entries."""
    n = len(h)
    a = np.frombuffer(h.encode("ascii", "replace"), np.uint8)
    ok = np.isin(a, np.frombuffer(b"ACGT", np.uint8))
    eq = np.zeros(n, bool)
    if n > u:
        eq[:n - u] = ok[:n - u] & ok[u:] & (a[:n - u] == a[u:])
    w = min(u, W_CAP)
    per = np.zeros(n, bool)
    m = n - u - w + 1                      # positions i with i + u + w <= n
    if m > 0:
        per[:m] = True
        for t in range(w):
            per[:m] &= eq[t:t + m]
    return per


def longest_run(per: np.ndarray) -> tuple[int, int]:
    """(start, length) of the longest run of True, the leftmost of equals; (0, 0) if there is none."""
    d = np.diff(np.concatenate(([0], per.astype(np.int8), [0])))
    starts, ends = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    if len(starts) == 0:
        return 0, 0
    k = int(np.argmax(ends - starts))          # (the first of equal maxima)
    return int(starts[k]), int(ends[k] - starts[k])


def unit_code(h: str, e: int, start: int, u: int) -> int:
    """The u letters from `start` as 2-bit codes.  A letter that is not ACGT (it can sit behind the unit's first 8 letters) carries
    the code the packed batch gives it: bits 1-2 of its ASCII letter, complemented at e = 1 like every other letter of that end."""
    code = 0
    for j in range(u):
        c = h[start + j]
        v = _CODE[c] if c in _CODE else ((ord(c) >> 1) & 3) ^ (2 if e == 1 else 0)
        code |= v << (2 * j)
    return code


def census_end(seq: str, e: int, u_min: int, u_max: int, lo: int, hi: int):
    """(hit tuple (unit, period, support, run_start, run_len, n_bases), [C_u]) of one read end."""
    h = end_string(seq, e, lo, hi)
    n = len(h)
    pers = {u: per_bits(h, u) for u in range(u_min, u_max + 1)}
    cs = [int(pers[u].sum()) for u in range(u_min, u_max + 1)]
    best = max(cs) if cs else 0
    if best == 0:
        return (0, 0, 0, 0, 0, 0), cs
    u = u_min + cs.index(best)
    start, length = longest_run(pers[u])
    return (unit_code(h, e, start, u), u, best, start, length, n), cs


def motif_census(seqs, u_min=4, u_max=32, lo=0, hi=1000, min_len=0, want_counts=False):
    """(hits MOTIF_HIT_DTYPE[n, 2], counts int32[n, 2, u_max - u_min + 1] or None), like HipScanner.motif_census."""
    n = len(seqs)
    hits = np.zeros((n, 2), hiplib.MOTIF_HIT_DTYPE)
    counts = np.zeros((n, 2, u_max - u_min + 1), np.int32)
    for r, seq in enumerate(seqs):
        if len(seq) <= min_len:
            continue
        for e in range(2):
            hit, cs = census_end(seq, e, u_min, u_max, lo, hi)
            hits[r, e] = hit + (0,)
            counts[r, e] = cs
    return hits, (counts if want_counts else None)
