"""Test helper: the placement rule (include/topsicle_hip.h, tps_window_place) and the naming of topsicle_amd/endref.py restated in
plain Python on string slices, dictionaries over k-mer strings and sorted lists.  Shares no code with the product: no hashes, no
sorted index, no directory, no histograms in bins of a wave.  (The coarse / fine end of a list of diagonals is the anchoring
oracle's: tests/anchor_oracle.py, offset_of.)"""
import numpy as np

import anchor_oracle as orc


def kmers_of(win, kept, k):
    """[(position, k-mer)] of a window's kept positions that hold k letters"""
    return [(p, win[p:p + k]) for p in sorted(kept) if 0 <= p <= len(win) - k]


def index_of(ref_windows, ref_keeps, k, max_occ):
    """k-mer -> [(r, q)] over all reference rows, the k-mers with more than max_occ entries left out"""
    idx = {}
    for r, (win, kept) in enumerate(zip(ref_windows, ref_keeps)):
        for q, s in kmers_of(win, kept, k):
            idx.setdefault(s, []).append((r, q))
    return {s: e for s, e in idx.items() if len(e) <= max_occ}


def place_one(idx, win, kept, k):
    """(ref, total, runner_ref, runner, offset, votes, second) of one query"""
    matches = [(r, q, p) for p, s in kmers_of(win, kept, k) for r, q in idx.get(s, ())]
    if not matches:
        return -1, 0, -1, 0, 0, 0, 0
    total = {}
    for r, _q, _p in matches:
        total[r] = total.get(r, 0) + 1
    ref = min(total, key=lambda r: (-total[r], r))
    others = {r: t for r, t in total.items() if r != ref}
    runner_ref = min(others, key=lambda r: (-others[r], r)) if others else -1
    offset, votes, second = orc.offset_of(sorted(q - p for r, q, p in matches if r == ref))
    return ref, total[ref], runner_ref, others.get(runner_ref, 0), offset, votes, second


def place_windows(windows, keeps, ref_windows, ref_keeps, k=12, max_occ=16):
    """The seven int32[n] arrays HipScanner.place_windows returns, from the windows as strings and their kept sets."""
    idx = index_of(ref_windows, ref_keeps, k, max_occ)
    out = np.zeros((7, len(windows)), np.int32)
    for i, (win, kept) in enumerate(zip(windows, keeps)):
        out[:, i] = place_one(idx, win, kept, k)
    return tuple(out)


# ---- the host rule of topsicle_amd/endref.py
def named(ref, votes, second, min_votes=20, ratio=4):
    return [r >= 0 and v >= min_votes and v >= ratio * s for r, v, s in zip(ref, votes, second)]


def group_names(end, name_of_read):
    """{group: (name index or None, agree, sorted other name indices, named members)}: the name most named members carry, ties to the
    reference end listed first (the smaller index).  name_of_read[i]: the index of the read's name, None where it has none."""
    out = {}
    for g in sorted(set(end) - {0}):
        mine = [name_of_read[i] for i in range(len(end)) if end[i] == g and name_of_read[i] is not None]
        if not mine:
            out[g] = (None, 0, [], 0)
            continue
        top = min(set(mine), key=lambda x: (-mine.count(x), x))
        out[g] = (top, mine.count(top), sorted(set(mine) - {top}), len(mine))
    return out
