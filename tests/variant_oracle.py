"""Test helper: the variant census restated from its definition (include/topsicle_hip.h, tps_batch_variant_census) in plain
Python / NumPy, one read, one rotation and one letter at a time -- no packed codes, no pieces, no lanes: nothing of the kernel's text.

For read r, h = the upper-cased read (tail 0) or its reverse complement (tail 1); end is clamped to L; a read with end - begin < m
contributes nothing.  Every i in [begin, end - m] is examined: x = h[i .. i + m); a letter that is not ACGT makes it "other";
else the smallest j with Hamming(x, R_j) <= 1 (R_j = the unit rotated left by j) decides: distance 0 canonical, distance 1 with the
mismatch at q the variant (p = (j + q) mod m, c = the letter x[q]).  The bin is min((end - 1 - i) // bin, n_bins - 1)."""
import numpy as np

_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
_CODE = {"A": 0, "C": 1, "T": 2, "G": 3}


def oriented(seq: str, tail: int) -> str:
    s = seq.upper()
    if tail == 1:
        s = s.encode("ascii", "replace").translate(_COMP)[::-1].decode("ascii")
    return s


def census_read(seq: str, unit: str, tail: int, begin: int, end: int, bin: int, n_bins: int):
    """(row int64[2 + 4m], profile int64[n_bins, 2 + 4m]) of one read."""
    m = len(unit)
    cols = 2 + 4 * m
    row = np.zeros(cols, np.int64)
    prof = np.zeros((n_bins, cols), np.int64)
    h = oriented(seq, tail)
    end = min(end, len(h))
    if end - begin < m:
        return row, prof
    a = np.frombuffer(h[begin:end].encode("ascii", "replace"), np.uint8)
    npos = end - begin - m + 1
    code = np.full(256, -1, np.int64)
    for c, v in _CODE.items():
        code[ord(c)] = v
    ca = code[a]
    valid = np.ones(npos, bool)
    for q in range(m):
        valid &= ca[q:q + npos] >= 0
    cls = np.zeros(npos, np.int64)                     # 0 = other
    decided = ~valid
    for j in range(m):
        rot = unit[j:] + unit[:j]
        mism = np.zeros(npos, np.int64)
        first_q = np.full(npos, -1, np.int64)
        for q in range(m):
            ne = a[q:q + npos] != ord(rot[q])
            first_q = np.where(ne & (mism == 0), q, first_q)
            mism += ne
        take0 = ~decided & (mism == 0)
        take1 = ~decided & (mism == 1)
        cls[take0] = 1
        i1 = np.nonzero(take1)[0]
        cls[i1] = 2 + 4 * ((j + first_q[i1]) % m) + ca[i1 + first_q[i1]]
        decided |= take0 | take1
    pos = begin + np.arange(npos)
    bins = np.minimum((end - 1 - pos) // bin, n_bins - 1)
    np.add.at(prof, (bins, np.zeros(npos, np.int64)), 1)
    hit = cls > 0
    np.add.at(prof, (bins[hit], cls[hit]), 1)
    return prof.sum(axis=0), prof


def variant_census(seqs, unit, tails, begin, end, bin=500, n_bins=40, want_profile=True):
    """(counts uint32[n, 2 + 4m], profile int64[n_bins, 2 + 4m] or None), like HipScanner.variant_census."""
    m = len(unit)
    counts = np.zeros((len(seqs), 2 + 4 * m), np.uint32)
    profile = np.zeros((n_bins, 2 + 4 * m), np.int64)
    for r, seq in enumerate(seqs):
        row, prof = census_read(seq, unit, int(tails[r]), int(begin[r]), int(end[r]), bin, n_bins)
        counts[r] = row
        profile += prof
    return counts, (profile if want_profile else None)
