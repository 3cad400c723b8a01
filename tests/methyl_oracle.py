"""The rules of `--methyl` in plain Python, on strings and lists: what tps_batch_mod_profile computes (mod_profile), what
tps_bam_mods_spans reads out of a BAM record's aux block (bam_mods), and the rows of methyl_{k}.csv.  Written from
include/topsicle_hip.h and include/topsicle_io.h alone; the kernel, its emulation and the native reader are compared with it bit for
bit."""
import struct

import numpy as np

from topsicle_amd import hiplib

MAX_REGION, MAX_BINS = 16384, 64
STATUS = ("ok", "none", "nogroup", "malformed", "clipped", "untagged")


def mod_profile(seqs, tails, begin, end, origin, mod_off, delta, prob, w=500, nb0=2, nb1=8, hi=205, lo=50):
    """(MOD_ROW_DTYPE[n], MOD_BIN_DTYPE[n, nb0 + nb1])"""
    n, nb = len(seqs), nb0 + nb1
    rows = np.zeros(n, hiplib.MOD_ROW_DTYPE)
    bins = np.zeros((n, nb), hiplib.MOD_BIN_DTYPE)
    for r, s in enumerate(seqs):
        s = s.upper()
        L = len(s)
        b, e = int(begin[r]), min(int(end[r]), L)
        if e <= b:
            continue
        t_of = (lambda p: L - 1 - p) if tails[r] else (lambda p: p)
        cs = [p for p in range(L) if s[p] == "C"]
        cpg = lambda p: p + 1 < L and s[p + 1] == "G"      # noqa: E731
        bin_of = lambda t: (t - int(origin[r])) // w + nb0      # noqa: E731  (Python's // is the floor)
        acc = [[0] * 5 for _ in range(nb)]
        for p in cs:
            if b <= t_of(p) < e and cpg(p):
                acc[bin_of(t_of(p))][0] += 1
        o, beyond, in_region, off = -1, 0, 0, 0
        for j in range(int(mod_off[r]), int(mod_off[r + 1])):
            o += int(delta[j]) + 1
            if o >= len(cs):
                beyond += 1
                continue
            p = cs[o]
            if not (b <= t_of(p) < e):
                continue
            in_region += 1
            if not cpg(p):
                off += 1
                continue
            a = acc[bin_of(t_of(p))]
            a[1] += 1
            a[2] += int(prob[j]) >= hi
            a[3] += int(prob[j]) <= lo
            a[4] += int(prob[j])
        if beyond:
            acc = [[0] * 5 for _ in range(nb)]
        rows[r] = (len(cs), int(mod_off[r + 1]) - int(mod_off[r]), beyond, in_region, off, sum(a[0] for a in acc), sum(a[1] for a in acc), 1 if beyond else 0)
        for k, a in enumerate(acc):
            bins[r, k] = tuple(a)
    return rows, bins


# ---- the aux block of a BAM record (SAMv1 4.2.4) and its MM / ML tags (SAMtags)
_FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def aux_tags(aux: bytes):
    """[(tag, type, value bytes)] or None where a tag runs past the block."""
    out, p = [], 0
    while p < len(aux):
        if p + 3 > len(aux):
            return None
        tag, typ = aux[p:p + 2].decode("latin1"), chr(aux[p + 2])
        p += 3
        if typ in _FIXED:
            n = _FIXED[typ]
        elif typ in "ZH":
            z = aux.find(b"\x00", p)
            if z < 0:
                return None
            n = z + 1 - p
        elif typ == "B":
            if p + 5 > len(aux) or chr(aux[p]) not in _FIXED or chr(aux[p]) == "A":
                return None
            n = 5 + _FIXED[chr(aux[p])] * struct.unpack_from("<I", aux, p + 1)[0]
        else:
            return None
        if p + n > len(aux):
            return None
        out.append((tag, typ, aux[p:p + n]))
        p += n
    return out


def parse_mm(mm: str):
    """[(base, strand, codes or None for a ChEBI number, flag, [counts])] by the SAMtags grammar, or None (a count over 2^32 - 1 too)."""
    groups, p = [], 0
    while p < len(mm):
        if mm[p] not in "ACGTUN" or p + 1 >= len(mm) or mm[p + 1] not in "+-":
            return None
        q = p + 2
        while q < len(mm) and mm[q].islower() and mm[q].isascii() and mm[q].isalpha():
            q += 1
        codes = mm[p + 2:q]
        if not codes:
            while q < len(mm) and mm[q].isdigit() and mm[q].isascii():
                q += 1
            if q == p + 2:
                return None
            codes = None
        flag = ""
        if q < len(mm) and mm[q] in ".?":
            flag = mm[q]
            q += 1
        counts = []
        while q < len(mm) and mm[q] == ",":
            d = q + 1
            while d < len(mm) and mm[d].isdigit() and mm[d].isascii():
                d += 1
            if d == q + 1:
                return None
            if int(mm[q + 1:d]) > 0xFFFFFFFF:
                return None
            counts.append(int(mm[q + 1:d]))
            q = d
        if q >= len(mm) or mm[q] != ";":
            return None
        groups.append((mm[p], mm[p + 1], codes, flag, counts))
        p = q + 1
    return groups


def record_mods(aux: bytes, l_seq: int, code: str = "m"):
    """(status, mode, [delta], [prob]) of one record's aux block; status as tps_bam_mods_spans numbers it."""
    tags = aux_tags(aux)
    if tags is None:
        return 3, 0, [], []
    mm = ml = mn = None
    for tag, typ, val in tags:
        if tag == "MM" and typ == "Z" and mm is None:
            mm = val[:-1].decode("latin1")
        elif tag == "ML" and typ == "B" and ml is None:
            if chr(val[0]) != "C":
                return 3, 0, [], []
            ml = list(val[5:])
        elif tag == "MN" and mn is None:
            if typ not in "cCsSiI":
                return 3, 0, [], []
            mn = int.from_bytes(val, "little", signed=typ in "csi")
    if mm is None or ml is None:
        return 1, 0, [], []
    groups = parse_mm(mm)
    if groups is None:
        return 3, 0, [], []
    at, found = 0, None
    for base, strand, codes, flag, counts in groups:
        n_codes = 1 if codes is None else len(codes)
        if found is None and base == "C" and strand == "+" and codes is not None and code in codes:
            found = (at, n_codes, codes.index(code), flag, counts)
        at += n_codes * len(counts)
    if found is None:
        return 2, 0, [], []
    if at > len(ml):
        return 3, 0, [], []
    if mn is not None and mn != l_seq:
        return 4, 0, [], []
    at, n_codes, which, flag, counts = found
    return 0, 1 if flag == "?" else 0, counts, [ml[at + i * n_codes + which] for i in range(len(counts))]


def thresholds(high: float, low: float):
    """(hi, lo): the smallest byte whose probability (ML + 0.5) / 256 is >= high, the largest whose is <= low."""
    import math
    return math.ceil(256 * high - 0.5), math.floor(256 * low - 0.5)
