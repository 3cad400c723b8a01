"""The cases tps_batch_mod_profile is checked on -- by the host emulation (tests/test_methyl.py), as a program under the sanitizers,
and on the GPU through the C ABI (tests/test_gpu_methyl.py) -- each against the plain rule of tests/methyl_oracle.py, computed once
per case and shared.  They are the smallest shapes at which the kernel can go wrong: reads shorter than, equal to and just over a
word of 16 bases; a CG across a word seam (every word is another lane's) and across the seam between two steps of 64 words; entry
lists around the scan's chunk of 64; ordinals at the read's first and last C, one past it, and far past 2^32; both tails; an origin
inside the region; clamped regions; the largest region and the most bins; a read of 70 000 bases with its region at the far end."""
import functools
import random

import numpy as np

import methyl_oracle as mo


class Case:
    def __init__(self, **kw):
        self.kw_ = dict(w=500, nb0=2, nb1=8, hi=205, lo=50)
        self.kw_.update(kw)
        self.reads, self.tails, self.begin, self.end, self.origin, self.ents = [], [], [], [], [], []

    def add(self, read, tail, begin, end, origin, ordinals=(), probs=None, deltas=None):
        """`ordinals`: which of the read's C's carry an entry (ascending, from 0); or the skip counts themselves."""
        if deltas is None:
            deltas, last = [], -1
            for o in ordinals:
                deltas.append(o - last - 1)
                last = o
        if probs is None:
            rng = random.Random(len(self.reads) * 7919 + len(deltas))
            probs = [rng.choice([0, 20, 49, 50, 51, 128, 204, 205, 206, 230, 255]) for _ in deltas]
        self.reads.append(read); self.tails.append(tail); self.begin.append(begin); self.end.append(end); self.origin.append(origin)
        self.ents.append((list(deltas), list(probs)))
        return self

    def kw(self):
        return dict(self.kw_)

    def lists(self, idx=None):
        """(mod_off, delta, prob) of the reads idx (all of them: None)"""
        ents = self.ents if idx is None else [self.ents[i] for i in idx]
        off = np.zeros(len(ents) + 1, np.int64)
        off[1:] = np.cumsum([len(d) for d, _ in ents])
        return off, np.array([x for d, _ in ents for x in d], np.uint32), np.array([x for _, p in ents for x in p], np.uint8)


def rand_read(rng, L, cpg=0.03, n_rate=0.002, lower=False):
    out = []
    while len(out) < L:
        x = rng.random()
        if x < cpg:
            out += ["C", "G"]
        elif x < cpg + n_rate:
            out.append("N")
        else:
            out.append(rng.choice("ACGT"))
    s = "".join(out[:L])
    return s.lower() if lower else s


def c_count(s):
    return s.upper().count("C")


def some(rng, s, share=0.5):
    """A random share of the read's C's, as ordinals."""
    return [o for o in range(c_count(s)) if rng.random() < share]


def _short():
    c = Case(w=16, nb0=1, nb1=3)
    rng = random.Random(11)
    for L in (1, 15, 16, 17, 33):
        for s in ("C" * L, ("CG" * L)[:L], ("GC" * L)[:L], rand_read(rng, L, cpg=0.3)):
            for tail in (0, 1):
                c.add(s, tail, 0, L, 0, range(c_count(s)))
    return c


def _no_c_last_c():
    c = Case(w=16, nb0=1, nb1=7)
    c.add("ATGGATTAGG" * 5, 0, 0, 50, 10)                                   # a read without a C
    c.add("ATGGATTAGG" * 5, 1, 0, 50, 10, [0])                              # ... and an entry all the same: beyond
    c.add("ATGGATTAGGCGTTAC", 0, 0, 16, 4, [0, 1])                          # the last base is C: no p + 1
    c.add("ATGGATTAGGCGTTAC", 1, 0, 16, 4, [0, 1])
    c.add("GTAAGATCGTTTTTTC", 0, 0, 16, 0, [1])
    return c


def _seams():
    c = Case(w=64, nb0=4, nb1=36)
    for at, behind in ((15, "G"), (15, "N"), (15, "g"), (31, "G"), (1023, "G"), (1023, "N"), (1183, "G"), (2047, "G")):
        s = list("AT" * 1100)
        s[at], s[at + 1] = "C", behind
        s[5], s[6] = "C", "G"
        s = "".join(s)
        for tail in (0, 1):
            c.add(s, tail, 0, 2200, 200, [0, 1])
            t_lo = 160 if tail == 0 else 2200 - 160 - 1120                   # a region whose 64th and 65th word meet at 1183 | 1184
            c.add(s, tail, t_lo, t_lo + 1120, t_lo + 200, [1])
    return c


def _entry_counts():
    c = Case(w=64, nb0=0, nb1=7)                                            # nb0 = 0
    s = "CG" * 200
    for n in (0, 1, 63, 64, 65, 129):
        c.add(s, 0, 0, 400, 0, range(n))
        c.add(s, 1, 3, 400, 3, range(200 - n, 200))
    c.add("ACG" + "T" * 90 + "CTCGA" + "T" * 20 + "CG", 0, 0, 120, 0, [0, 3])             # the first and the last C
    c.add("ACG" + "T" * 90 + "CTCGA" + "T" * 20 + "CG", 0, 0, 120, 0, [0, 4])             # beyond by exactly one
    c.add("ACG" + "T" * 90 + "CTCGA" + "T" * 20 + "CG", 1, 0, 120, 0, [1, 2, 3, 4, 5])
    c.add("CG" * 50, 0, 0, 100, 0, deltas=[0, 0xFFFFFFFF, 0xFFFFFFFF, 0], probs=[255, 255, 255, 255])      # 2^32 - 1 twice: no wrap
    c.add("CG" * 50, 0, 0, 100, 0, deltas=[0xFFFFFFFF] * 70, probs=[1] * 70)
    return c


def _regions():
    c = Case(w=500, nb0=2, nb1=4)
    rng = random.Random(5)
    s = rand_read(rng, 3000)
    ents = some(rng, s)
    for tail in (0, 1):
        c.add(s, tail, 100, 2100, 613, ents)                                 # mirrored regions; t - origin = -513 .. : floor, not truncation
        c.add(s, tail, 101, 2613, 613, ents)                                 # begin no multiple of 16
        c.add(s, tail, 0, 1 << 30, 1000, ents)                               # clamped at the read's start and at its end
        c.add(s, tail, 2999, 5000, 2999, ents)
        c.add(s, tail, 3000, 5000, 0, ents)                                  # behind the read: empty after the clamp
        c.add(s, tail, 700, 700, 0, ents)                                    # begin = end
    low = rand_read(rng, 2000, lower=True)
    c.add(low, 0, 0, 2000, 1000, some(rng, low))
    return c


def _most_bins():
    c = Case(w=16, nb0=20, nb1=44, hi=1, lo=0)
    rng = random.Random(6)
    s = rand_read(rng, 1500, cpg=0.2)
    for tail in (0, 1):
        c.add(s, tail, 80, 1104, 400, some(rng, s, 0.8))
        c.add(s, tail, 399, 401, 400, some(rng, s, 0.8))
    return c


def _largest():
    c = Case(w=4096, nb0=1, nb1=4, hi=255, lo=254)
    rng = random.Random(7)
    s = rand_read(rng, 20000, cpg=0.1)
    c.add(s, 0, 1000, 17384, 3000, some(rng, s, 0.7))                        # exactly 16 384 bases
    c.add(s, 1, 1007, 17391, 5000, some(rng, s, 0.7))
    c.add("CG" * 10000, 0, 3616, 20000, 3616 + 4096, range(10000), probs=[255] * 10000)    # the fullest bins there can be
    return c


def _long():
    c = Case(w=500, nb0=1, nb1=9)
    rng = random.Random(8)
    s = rand_read(rng, 70000)
    c.add(s, 1, 100, 5100, 600, some(rng, s, 0.5))                           # the region at the read's far end, entries on either side
    c.add(s, 0, 100, 5100, 600, some(rng, s, 0.02))
    return c


def _mixed():
    c = Case(w=500, nb0=2, nb1=8)
    rng = random.Random(9)
    for i in range(40):
        L = rng.choice([1, 16, 17, 63, 64, 65, 1000, 1023, 1024, 1025, 4000, 6000, 9000])
        s = rand_read(rng, L, cpg=rng.choice([0.0, 0.02, 0.2]), lower=i % 9 == 4)
        ents = some(rng, s, rng.choice([0.0, 0.1, 1.0]))
        if i % 7 == 3 and ents:
            ents.append(c_count(s) + i)                                      # a tag that does not belong to these bases
        origin = rng.randrange(0, L + 1)
        if i % 5 == 2:
            c.add(s, 0, 0, 0, origin, ents)                                  # the empty region
        else:
            c.add(s, rng.randrange(2), max(0, origin - rng.randrange(0, 1001)), origin + rng.randrange(0, 4001), origin, ents)
    return c


CASES = {"short": _short, "no_c_last_c": _no_c_last_c, "seams": _seams, "entry_counts": _entry_counts, "regions": _regions, "most_bins": _most_bins,
         "largest": _largest, "long": _long, "mixed": _mixed}


def names():
    return list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    rows, bins = mo.mod_profile(c.reads, c.tails, c.begin, c.end, c.origin, *c.lists(), **c.kw())
    rows.setflags(write=False)
    bins.setflags(write=False)
    return rows, bins


def assert_equal(got, name, idx=None):
    rows, bins = expected(name)
    if idx is not None:
        rows, bins = rows[idx], bins[idx]
    for r in range(len(rows)):
        assert got[0][r] == rows[r], (name, r, got[0][r], rows[r])
        assert np.array_equal(got[1][r], bins[r]), (name, r, got[1][r], bins[r])
    assert np.array_equal(got[0], rows) and np.array_equal(got[1], bins)


# (keyword overrides of the good call, the return code, words of the message): every refusal of tps_batch_mod_profile
REFUSALS = [
    (dict(w=15), "rc=-5", "w must be 16..4096"),
    (dict(w=4097), "rc=-5", "w must be 16..4096"),
    (dict(nb0=0, nb1=0), "rc=-5", "nb0 + nb1 must be 1..64"),
    (dict(nb0=-1, nb1=4), "rc=-5", "nb0 + nb1 must be 1..64"),
    (dict(nb0=32, nb1=33), "rc=-5", "nb0 + nb1 must be 1..64"),
    (dict(hi=50, lo=50), "rc=-3", "lo < hi"),
    (dict(hi=256), "rc=-3", "lo < hi"),
    (dict(lo=-1), "rc=-3", "lo < hi"),
    (dict(n_reads=2), "rc=-3", "must hold 1 reads"),
    (dict(rows_len=2), "rc=-3", "rows must hold 1 rows"),
    (dict(bins_len=9), "rc=-3", "bins must hold 10 records"),
    (dict(tails=[2]), "rc=-3", "read 0: tail must be 0 or 1"),
    (dict(begin=[-1]), "rc=-3", "read 0: need 0 <= begin <= end"),
    (dict(begin=[60], end=[50]), "rc=-3", "read 0: need 0 <= begin <= end"),
    (dict(origin=[-1]), "rc=-3", "read 0: origin must not be negative"),
    (dict(mod_off=[2, 1]), "rc=-3", "read 0: mod_off must ascend"),
    (dict(mod_off=[-1, 2]), "rc=-3", "mod_off must not be negative"),
    (dict(mod_off=[0, 1]), "rc=-3", "mod_off must end at n_mods = 2"),
    (dict(origin=[1100], begin=[99]), "rc=-3", "read 0: the region leaves the bins"),
    (dict(origin=[0], w=16, nb1=6), "rc=-3", "read 0: the region leaves the bins"),
]
# ... and the one that needs a long read: a region over 16 384 bases (w = 4096, nb0 = 0, nb1 = 5, origin = 0)
LONG_REFUSAL = (dict(begin=[0, 0], end=[16384, 16385]), "rc=-5", "read 1: end - begin must be at most 16384")


# ---- the aux walk: records made by tests/bam_tools.record_bytes, their aux blocks written here byte by byte
def aux(tag, typ, payload=b""):
    return tag.encode() + typ.encode() + payload


def aux_b(tag, sub, values):
    import struct
    fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub]
    return aux(tag, "B", sub.encode() + struct.pack("<i", len(values)) + struct.pack("<%d%s" % (len(values), fmt), *values))


def mm(text):
    return aux("MM", "Z", text.encode() + b"\x00")


def ml(values):
    return aux_b("ML", "C", values)


def _every_type():
    import struct
    return (aux("XA", "A", b"Q") + aux("Xc", "c", b"\xff") + aux("XC", "C", b"\x07") + aux("Xs", "s", struct.pack("<h", -300)) + aux("XS", "S", struct.pack("<H", 60000)) +
            aux("Xi", "i", struct.pack("<i", -70000)) + aux("XI", "I", struct.pack("<I", 4000000000)) + aux("Xf", "f", struct.pack("<f", 1.5)) +
            aux("XZ", "Z", b"MM:Z:C+m?,9;\x00") + aux("XH", "H", b"1AE301\x00") + aux_b("Xb", "c", [-1, 2]) + aux_b("XB", "S", [1, 2, 3]) + aux_b("Xg", "f", [0.5]) +
            aux_b("XM", "C", [9, 9, 9]))


# (name, aux block, (status, mode, deltas, probs) written out by hand, code asked for)
AUX_CASES = [
    ("every_type_in_front", _every_type() + mm("C+m?,1,0,2;") + ml([10, 200, 30]), (0, 1, [1, 0, 2], [10, 200, 30]), "m"),
    ("ml_in_front_of_mm", ml([7, 8]) + aux("RG", "Z", b"x\x00") + mm("C+m.,5,6;"), (0, 0, [5, 6], [7, 8]), "m"),
    ("explicit", mm("C+m?,0,0;") + ml([1, 2]), (0, 1, [0, 0], [1, 2]), "m"),
    ("implicit_dot", mm("C+m.,3;") + ml([250]), (0, 0, [3], [250]), "m"),
    ("implicit_no_flag", mm("C+m,3,4;") + ml([250, 4]), (0, 0, [3, 4], [250, 4]), "m"),
    ("two_codes_first", mm("C+mh?,1,2;") + ml([11, 12, 21, 22]), (0, 1, [1, 2], [11, 21]), "m"),
    ("two_codes_second", mm("C+mh?,1,2;") + ml([11, 12, 21, 22]), (0, 1, [1, 2], [12, 22]), "h"),
    ("two_codes_swapped", mm("C+hm,1,2;") + ml([11, 12, 21, 22]), (0, 0, [1, 2], [12, 22]), "m"),
    ("two_codes_swapped_h", mm("C+hm,1,2;") + ml([11, 12, 21, 22]), (0, 0, [1, 2], [11, 21]), "h"),
    ("second_group", mm("C+h?,4,4,4;C+m?,0,7;") + ml([1, 2, 3, 90, 91]), (0, 1, [0, 7], [90, 91]), "m"),
    ("other_groups_around", mm("A+a.,1;N+n?,2,2;C+76792,0;C-m?,5;C+m.,8;T+g,1;") + ml([1, 2, 3, 4, 5, 66, 7]), (0, 0, [8], [66]), "m"),
    ("first_of_two_on_c", mm("C+m?,1;C+m.,2;") + ml([5, 6]), (0, 1, [1], [5]), "m"),
    ("base_n", mm("N+m?,1;") + ml([5]), (2, 0, [], []), "m"),
    ("minus_strand", mm("C-m?,1;") + ml([5]), (2, 0, [], []), "m"),
    ("chebi_only", mm("C+76792?,1;") + ml([5]), (2, 0, [], []), "m"),
    ("other_code", mm("C+h?,1;") + ml([5]), (2, 0, [], []), "m"),
    ("empty_tag", mm("") + ml([]), (2, 0, [], []), "m"),
    ("empty_list", mm("C+m?;") + ml([]), (0, 1, [], []), "m"),
    ("largest_count", mm("C+m?,4294967295,4294967295;") + ml([1, 2]), (0, 1, [4294967295, 4294967295], [1, 2]), "m"),
    ("ml_one_short", mm("C+m?,1,2,3;") + ml([1, 2]), (3, 0, [], []), "m"),
    ("ml_short_behind_the_group", mm("C+m?,1;C+h?,1,1;") + ml([1, 2]), (3, 0, [], []), "m"),
    ("count_two_to_32", mm("C+m?,4294967296;") + ml([1]), (3, 0, [], []), "m"),
    ("count_of_30_digits", mm("C+m?," + "9" * 30 + ";") + ml([1]), (3, 0, [], []), "m"),
    ("non_digit", mm("C+m?,1x;") + ml([1]), (3, 0, [], []), "m"),
    ("no_semicolon", mm("C+m?,1") + ml([1]), (3, 0, [], []), "m"),
    ("empty_count", mm("C+m?,,1;") + ml([1, 2]), (3, 0, [], []), "m"),
    ("ml_of_shorts", mm("C+m?,1;") + aux_b("ML", "S", [1]), (3, 0, [], []), "m"),
    ("mn_equal", mm("C+m?,1;") + ml([9]) + aux("MN", "i", (60).to_bytes(4, "little")), (0, 1, [1], [9]), "m"),
    ("mn_differs", mm("C+m?,1;") + ml([9]) + aux("MN", "i", (75).to_bytes(4, "little")), (4, 0, [], []), "m"),
    ("mn_differs_as_short", aux("MN", "S", (59).to_bytes(2, "little")) + mm("C+m?,1;") + ml([9]), (4, 0, [], []), "m"),
    ("ml_without_mm", ml([1, 2, 3]), (1, 0, [], []), "m"),
    ("mm_without_ml", mm("C+m?,1;"), (1, 0, [], []), "m"),
    ("no_aux", b"", (1, 0, [], []), "m"),
    ("tag_past_the_record", mm("C+m?,1;") + ml([9]) + aux("XI", "I", b"\x01\x02"), (3, 0, [], []), "m"),
    ("string_without_end", ml([9]) + aux("MM", "Z", b"C+m?,1;"), (3, 0, [], []), "m"),
    ("array_past_the_record", mm("C+m?,1;") + aux("ML", "B", b"C" + (5).to_bytes(4, "little") + b"\x01\x02"), (3, 0, [], []), "m"),
    ("unknown_type", aux("XX", "q", b"\x00") + mm("C+m?,1;") + ml([9]), (3, 0, [], []), "m"),
    ("at_the_end_of_the_window", mm("C+m.,2,2;") + ml([3, 4]), (0, 0, [2, 2], [3, 4]), "m"),
]
AUX_SEQ = "ACGT" * 15                                            # l_seq = 60


def aux_window(cases=None):
    """(text, spans int64[n, 4], lens int32[n]): the records of AUX_CASES behind one another as the reader's window holds them, the
    last one ending at the window's very end."""
    import struct
    import bam_tools
    text, spans = [b"\x00" * 7], []
    at = 7
    for i, (name, block, _want, _code) in enumerate(AUX_CASES if cases is None else cases):
        flag, cigar = (bam_tools.FLAG_REVERSE, [(60, "M")]) if i % 3 == 1 else (bam_tools.FLAG_UNMAPPED, [])
        rec = bam_tools.record_bytes(name, flag, AUX_SEQ, "I" * 60 if i % 4 else None, ref_id=0 if cigar else -1, pos=5 if cigar else -1, cigar=cigar)
        body = rec[4:] + block
        rec = struct.pack("<i", len(body)) + body
        h0 = at + 36
        s0 = h0 + len(name) + 1 + 4 * len(cigar)
        spans.append((h0, len(name), s0, s0 + 30))
        text.append(rec)
        at += len(rec)
    return b"".join(text), np.array(spans, np.int64), np.full(len(spans), 60, np.int32)


# ---- end to end: a BAM of 60 reads of 6000 bases, 40 of them telomeric, CpGs planted every 40 .. 120 bases of subtelomere
def cli_bam_reads(n=60, L=6000, seed=21):
    """[(name, flag, read as sequenced, qual, cigar, tags)] as bam_tools.write_bam takes them, and per read (kind, planted tract):
    kind `high` / `low` (every CpG called with ML >= 230 / <= 20), `none` (no tags), `malformed`, `other` (not telomeric)."""
    import bam_tools
    rng = random.Random(seed)
    reads, truth = [], []
    for i in range(n):
        telomeric = i % 3 != 2
        tract = rng.randrange(100, 400) * 6 if telomeric else 0
        body = [rng.choice("ACGT") for _ in range(L - tract)]
        for j in range(1, len(body)):
            if body[j - 1] == "C" and body[j] == "G":
                body[j] = "T"
        j = rng.randrange(40, 121)
        while telomeric and j + 1 < len(body):
            body[j], body[j + 1] = "C", "G"
            j += rng.randrange(40, 121)
        h = "CCCTAA" * (tract // 6) + "".join(body)              # (the tract holds no CG and ends in A: none across the boundary either)
        s =bam_tools.revcomp(h) if i % 4 == 1 else h             # a quarter with the telomere at the far end: tail 1
        cs = [p for p, c in enumerate(s) if c == "C"]
        sites = [o for o, p in enumerate(cs) if p + 1 < L and s[p + 1] == "G"]
        deltas, last = [], -1
        for o in sites:
            deltas.append(o - last - 1)
            last = o
        n_tel = sum(1 for t in truth if t[0] in ("high", "low"))
        kind = "other" if not telomeric else "none" if i in (7, 22) else "malformed" if i == 13 else "high" if n_tel % 2 == 0 else "low"
        probs = [rng.randrange(230, 256) if kind == "high" else rng.randrange(0, 21) for _ in sites]
        flag_mode = "?" if i % 5 else "."
        tags = [("RG", "Z", "run1_model"), ("qs", "f", 12.5)]
        if kind == "malformed":
            tags += [("MM", "Z", "C+m?" + "".join(f",{x}" for x in deltas) + ";"), ("ML", "B", ("C", probs[:-1]))]
        elif kind != "none":
            tags += [("MM", "Z", f"C+h?;C+m{flag_mode}" + "".join(f",{x}" for x in deltas) + ";"), ("ML", "B", ("C", probs)), ("MN", "i", L)]
        flag, cigar = (bam_tools.FLAG_REVERSE, [(L, "M")]) if i % 3 == 0 else (0, [(L, "M")]) if i % 3 == 1 else (bam_tools.FLAG_UNMAPPED, [])
        reads.append((f"read{i}", flag, s, "I" * L, cigar, tags))
        truth.append((kind, tract, deltas, probs, flag_mode))
    return reads, truth


def check_cli_outputs(outdir, reads, truth, ks, bin_w=500, bins=8, tract=2, high=0.8, low=0.2):
    """Every row of methyl_{k}.csv equals the plain rule applied to that read with the boundary telolengths_all.csv stores for it, one
    row per stored boundary, in run order.  Returns the rows of the first k as dicts."""
    import csv
    import os
    from topsicle_amd import methyl
    hi, lo = mo.thresholds(high, low)
    by_name = {r[0]: (r, t) for r, t in zip(reads, truth)}
    telo = list(csv.DictReader(open(os.path.join(outdir, "telolengths_all.csv"))))
    first = None
    for k in ks:
        stored = {r["readID"]: int(float(r["telo_length"])) for r in telo if int(r["phrase"]) == k and float(r["telo_length"]) != 0}
        rows = list(csv.reader(open(os.path.join(outdir, f"methyl_{k}.csv"))))
        assert rows[0] == methyl.READ_HEADER
        assert [r[1] for r in rows[1:]] == [r["readID"] for r in telo if int(r["phrase"]) == k and r["readID"] in stored]
        for r in rows[1:]:
            (name, _flag, s, _q, _cigar, _tags), (kind, _tract, deltas, probs, flag_mode) = by_name[r[1]]
            tail = {"forward": 0, "reverse": 1}[r[2]]
            origin = stored[r[1]]
            assert int(r[3]) == origin
            if kind in ("none", "malformed"):
                assert r[4:] == [kind] + [""] * 10, r
                continue
            row, bn = mo.mod_profile([s], [tail], [max(0, origin - tract * bin_w)], [origin + bins * bin_w], [origin], [0, len(deltas)], deltas, probs,
                                     w=bin_w, nb0=tract, nb1=bins, hi=hi, lo=lo)
            behind = bn[0][tract:]
            cpg, called, n_hi, n_lo, total = (int(behind[f].sum()) for f in ("cpg", "called", "high", "low", "sum"))
            den = n_hi + n_lo + (cpg - called if flag_mode == "." else 0)
            want = ["ok", "explicit" if flag_mode == "?" else "implicit", str(row[0]["c_total"]), str(len(deltas)), str(row[0]["off_context"]), str(cpg), str(called),
                    str(n_hi), str(n_lo), "" if den == 0 else "%.4f" % (n_hi / den), "" if called == 0 else "%.4f" % ((total / called + 0.5) / 256)]
            assert r[4:] == want, (k, r[1], r[4:], want)
        if first is None:
            first = [dict(zip(rows[0], r)) for r in rows[1:]]
    return first
