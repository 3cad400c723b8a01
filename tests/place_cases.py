"""Test helper: the query and reference windows of the placement tests (tests/test_place.py on the host emulation,
tests/test_gpu_place.py on the GPU), the planted-end reference, and the oracle's answers to all of them, computed once per process
(tests/place_oracle.py)."""
import functools

import numpy as np

import anchor_cases as ac
import anchor_oracle as orc
import ends_cases as ec
import ends_oracle as eo
import place_oracle as po
from tract_cases import repeats

OUTPUTS = ("ref", "total", "runner_ref", "runner", "offset", "votes", "second")


class Case:
    """Query windows and reference windows as strings with their kept sets."""

    def __init__(self, name, k=12, span=2000, max_occ=16):
        self.name, self.k, self.span, self.max_occ = name, k, span, max_occ
        self.windows, self.keeps, self.ref_windows, self.ref_keeps = [], [], [], []

    def _all(self, win, kept):
        return set(range(max(0, len(win) - self.k + 1))) if kept is None else set(kept)

    def query(self, win, kept=None):
        self.windows.append(win)
        self.keeps.append(self._all(win, kept))
        return len(self.windows) - 1

    def ref(self, win, kept=None):
        self.ref_windows.append(win)
        self.ref_keeps.append(self._all(win, kept))
        return len(self.ref_windows) - 1


LENGTHS = (0, 11, 12, 75, 76, 77, 4096)            # (k = 12: k - 1, k; 64 positions - 1, 64, 65; the longest)


def _lengths_case():
    """Queries of 0 .. 4096 letters cut from the front of reference row 1; the longest equals its reference."""
    rng = np.random.default_rng(601)
    c = Case("lengths", span=4096)
    R = ec.rand(rng, 4096)
    c.ref(ec.rand(rng, 500))
    c.ref(R)
    for n in LENGTHS:
        c.query(R[:n])
    return c


def _empty_refs_case():
    """A reference row without letters, one whose keep bits are all clear, one shorter than k, and one that is matched."""
    rng = np.random.default_rng(602)
    c = Case("empty_refs", span=300)
    A, B = ec.rand(rng, 300), ec.rand(rng, 300)
    c.ref("")
    c.ref(A, kept=set())
    c.ref(B[:11])
    c.ref(B)
    c.query(A)                                     # its row has no kept position: no match
    c.query(B[20:220])
    c.query(A[:150] + B[150:])
    c.query(A, kept=set())
    return c


def _single_case():
    """R = 1, n = 1: no runner-up."""
    rng = np.random.default_rng(603)
    c = Case("single", span=200)
    R = ec.rand(rng, 200)
    c.ref(R)
    c.query(ec.rand(rng, 7) + R[:150])
    return c


def _many_refs_case():
    """R = 1024 rows of 21 k-mers each, n = 13 (no multiple of a workgroup's waves): the first row, the last, two rows in one query."""
    rng = np.random.default_rng(604)
    c = Case("many_refs", span=32)
    rows = [ec.rand(rng, 32) for _ in range(1024)]
    for r in rows:
        c.ref(r)
    for r in (0, 1023, 1, 63, 64, 65, 512, 1022):
        c.query(rows[r][3:])
    c.query(rows[1023][:16] + rows[0][:16])        # equal totals: row 0
    c.query(rows[700][:20] + rows[900][:12])
    c.query(rows[5][:12] + rows[6][:12])           # one k-mer each, the smaller row; the runner-up is the other
    c.query(ec.rand(rng, 32))
    c.query(rows[1023], kept={20})
    return c


def _occ_case(max_occ):
    """A k-mer with exactly max_occ entries (it votes for every row that holds it) and one with max_occ + 1 (dropped whole); the last
    entry of the second lies twice in ONE row, and so do two of the first's where max_occ allows."""
    rng = np.random.default_rng(610 + max_occ)
    c = Case(f"occ{max_occ}", span=100, max_occ=max_occ)
    A, B = ec.rand(rng, 12), ec.rand(rng, 12)
    n_rows = max_occ + 1
    for r in range(n_rows):
        fill = ec.rand(rng, 40)
        a = A if r < max_occ - (1 if max_occ > 1 else 0) else ""
        if max_occ > 1 and r == 0:
            a = A + "C" + A                        # twice in one row
        b = B if r < max_occ - 1 else ""
        if r == max_occ:
            b = B + "G" + B                        # twice in one row: max_occ + 1 entries in all
        c.ref(fill[:20] + a + "T" + b + fill[20:])
    c.query("ACGT" + A, kept={4})
    c.query("ACGT" + B, kept={4})                  # dropped: no match
    c.query("ACGT" + A + "T" + B)
    c.query(c.ref_windows[max_occ])                # the row that holds B twice: its own k-mers place it
    c.query(c.ref_windows[0])
    return c


def _ties_case():
    """Equal totals on two rows (the smaller r wins), equal runner-ups (the smaller r), a query that matches one row only."""
    rng = np.random.default_rng(605)
    c = Case("ties", span=200)
    rows = [ec.rand(rng, 200) for _ in range(4)]
    for r in rows:
        c.ref(r)
    c.query(rows[2][:40] + rows[1][:40])
    c.query(rows[3][:50] + rows[2][:40] + rows[1][:40])
    c.query(rows[2][:60])
    c.query(rows[1][100:140] + rows[3][:41])
    c.query(rows[0][:40] + rows[0][180:])          # two diagonals of one row, two coarse bins apart: `second`
    return c


def _extreme_case(k):
    """The extreme diagonals d = +-(4096 - k): a query's last kept k-mer against a reference's first, and the other way round."""
    rng = np.random.default_rng(620 + k)
    c = Case(f"extreme_k{k}", k=k, span=4096)
    R0, R1 = ec.rand(rng, 4096), ec.rand(rng, 4096)
    c.ref(R0, kept={0})
    c.ref(R1, kept={4096 - k})
    c.query(ec.rand(rng, 4096 - k) + R0[:k], kept={4096 - k})
    c.query(R1[4096 - k:] + ec.rand(rng, 4096 - k), kept={0})
    return c


_LETTERS = "ACTG"                                  # code 0 1 2 3


def _kmer_with_hash(x, k=12):
    """The k-mer whose hash is x, None where its code has more than 2 k bits (fmix32 undone step by step)."""
    m = 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7ED1B41D) & m                       # the inverse of 0xC2B2AE35 mod 2^32
    x ^= (x >> 13) ^ (x >> 26)
    x = (x * 0xA5CB9243) & m                       # the inverse of 0x85EBCA6B
    x ^= x >> 16
    c = x ^ 0x9E3779B9
    if c >> (2 * k):
        return None
    return "".join(_LETTERS[(c >> (2 * q)) & 3] for q in range(k))


def bucket_kmers(k=12):
    """k-mers whose hashes have the top 16 bits 0x0000, 0x0000 (another one), 0x7FFF, 0x8000 and 0xFFFF: the first bucket, both sides
    of the border in the middle and the last bucket of a directory of up to 16 bits."""
    out = []
    for top, skip in ((0x0000, 0), (0x0000, 1), (0x7FFF, 0), (0x8000, 0), (0xFFFF, 0)):
        found = [s for s in (_kmer_with_hash((top << 16) | low, k) for low in range(65536)) if s is not None]
        s = found[skip]
        assert eo.kmer_hash(s) >> 16 == top
        out.append(s)
    return out


def _buckets_case():
    """Hashes in the first and in the last bucket of the directory and on both sides of a bucket border, beside 3 000 other k-mers;
    two k-mers of the first bucket, one of them absent from the reference (the look-up walks past its neighbour)."""
    rng = np.random.default_rng(606)
    c = Case("buckets", span=3100)
    first, first2, below, above, last = bucket_kmers()
    c.ref(ec.rand(rng, 3000))
    c.ref(first + below + above + last, kept={0, 12, 24, 36})
    c.ref(above + first, kept={0, 12})
    for s in (first, first2, below, above, last):
        c.query("AC" + s, kept={2})
    c.query(last + first2 + above + below + first, kept={0, 12, 24, 36, 48})
    c.query(c.ref_windows[0][100:400])
    return c


def _reads_case(name, rows):
    """Windows extracted from reads on both tails (and with N, other letters and lower case): the anchoring tests' own, the rows
    `rows` of them as the reference."""
    src, want = ac.case(name), ac.expected(name)
    c = Case(f"reads_{name}", k=src.k, span=src.span)
    for win, kept in zip(want["windows"], want["keeps"]):
        c.query(win, kept)
    for r in rows:
        c.ref(want["windows"][r], want["keeps"][r])
    return c


@functools.lru_cache(maxsize=None)
def cases():
    out = [_lengths_case(), _empty_refs_case(), _single_case(), _many_refs_case(), _occ_case(1), _occ_case(2), _occ_case(16), _ties_case()]
    out += [_extreme_case(8), _extreme_case(12), _extreme_case(16), _buckets_case()]
    out += [_reads_case("letters", (0, 6)), _reads_case("unit_CCCTAA", (0, 3, 6)), _reads_case("k8_span1999", (0, 3, 6)), _reads_case("k16_span2001", (0, 3, 6))]
    return tuple(out)


CASE_IDS = [c.name for c in cases()]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def rows(name):
    """(codes, keep, length, ref_codes, ref_keep, ref_length) of case `name`, as HipScanner.place_windows takes them."""
    c = case(name)
    return orc.pack(c.windows, c.keeps, c.span) + orc.pack(c.ref_windows, c.ref_keeps, c.span)


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    return po.place_windows(c.windows, c.keeps, c.ref_windows, c.ref_keeps, c.k, c.max_occ)


def assert_equal(got, want, name):
    assert len(got) == len(want) == 7
    for what, g, w in zip(OUTPUTS, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype == np.int32, (name, what, g.shape, w.shape, g.dtype)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, f"{name}: {what} differs at rows {bad[:5].tolist()}: got {g[bad[0]]}, want {w[bad[0]]}"


def run_case(place_windows, name):
    """The seven arrays of `place_windows` (an engine's or a driver's) on case `name`."""
    c = case(name)
    return place_windows(*rows(name), c.span, c.k, c.max_occ)


# ---- the refusals: (what differs from a good call, the return code in the message).  lens = (codes_len, keep_len, n, ref_codes_len,
# ref_keep_len, n_ref, out_len); rows of 7 and 4 dwords, two queries, three reference rows
GOOD = dict(length=[100, 5], ref_length=[100, 0, 50], span=100, k=12, max_occ=16, lens=None)
GOOD_LENS = (14, 8, 2, 21, 12, 3, 2)


def _lens(**kw):
    at = dict(codes_len=0, keep_len=1, n=2, ref_codes_len=3, ref_keep_len=4, n_ref=5, out_len=6)
    out = list(GOOD_LENS)
    for key, v in kw.items():
        out[at[key]] = v
    return tuple(out)


REFUSALS = [
    (dict(lens=_lens(n=262145, codes_len=262145 * 7, keep_len=262145 * 4, out_len=262145)), "rc=-5"),
    (dict(lens=_lens(n_ref=0, ref_codes_len=0, ref_keep_len=0)), "rc=-5"), (dict(lens=_lens(n_ref=1025, ref_codes_len=1025 * 7, ref_keep_len=1025 * 4)), "rc=-5"),
    (dict(span=11), "rc=-5"), (dict(span=4097), "rc=-5"), (dict(k=7), "rc=-5"), (dict(k=17), "rc=-5"), (dict(max_occ=0), "rc=-5"), (dict(max_occ=65), "rc=-5"),
    (dict(length=[101, 5]), "rc=-3"), (dict(length=[-1, 5]), "rc=-3"), (dict(ref_length=[100, 0, 101]), "rc=-3"), (dict(ref_length=[-1, 0, 50]), "rc=-3"),
    (dict(lens=_lens(codes_len=13)), "rc=-3"), (dict(lens=_lens(keep_len=9)), "rc=-3"), (dict(lens=_lens(ref_codes_len=14)), "rc=-3"),
    (dict(lens=_lens(ref_keep_len=8)), "rc=-3"), (dict(lens=_lens(out_len=1)), "rc=-3"), (dict(lens=_lens(n=1)), "rc=-3"), (dict(lens=_lens(n_ref=2)), "rc=-3"),
]
REFUSAL_ROWS = dict(codes=np.zeros((2, 7), np.uint32), keep=np.zeros((2, 4), np.uint32), ref_codes=np.zeros((3, 7), np.uint32), ref_keep=np.zeros((3, 4), np.uint32))


# ---- detection: the planted ends of tests/ends_cases.py against a reference of five of them and a decoy
REF_ENDS, REF_TELO, DECOY = 5, 2500, "decoy"
SPACER = 25000                                     # between the two ends of a record: more than maxlengthtelo, a piece holds one telomere
MIN_VOTES, RATIO = 20, 4                           # the defaults of topsicle_amd.endref


@functools.lru_cache(maxsize=None)
def detection_subs(ident):
    """The planted subtelomeres of the set: the first draws of its seeded generator (ends_cases.detection_reads)."""
    motif, err = ident.rsplit("_", 1)
    rng = np.random.default_rng(ec.DETECT[motif][0 if err == "ONT" else 1])
    return [ec.rand(rng, ec.READ_LEN + 600) for _ in range(ec.N_ENDS)]


@functools.lru_cache(maxsize=None)
def detection_reference(ident):
    """([(record id, sequence)], {piece name: planted end 1 .. 5 or DECOY}): ends 1 - 5 (end 6 is left out) and one decoy that shares
    1 000 of its first 2 000 subtelomere bases with end 1 at the same place, each behind 2 500 error-free bases of the motif, two to
    a record -- head, random sequence, reverse-complemented tail -- so that both sides and both tails occur."""
    motif = ident.rsplit("_", 1)[0]
    subs = detection_subs(ident)
    rng = np.random.default_rng(7000 + ec.DETECT_IDS.index(ident))
    decoy = ec.rand(rng, 500) + subs[0][500:1500] + ec.rand(rng, 3500)
    ends = [(e + 1, repeats(motif, REF_TELO, e) + subs[e][:5000]) for e in range(REF_ENDS)] + [(DECOY, repeats(motif, REF_TELO, 2) + decoy)]
    records, truth = [], {}
    for j in range(0, len(ends), 2):
        (e0, head), (e1, tail) = ends[j], ends[j + 1]
        rid = f"chr{j // 2 + 1}"
        records.append((rid, head + ec.rand(rng, SPACER) + ec.stored_revcomp(tail)))
        truth[f"{rid}_head"], truth[f"{rid}_tail"] = e0, e1
    return records, truth


def write_reference(path, ident):
    records, _truth = detection_reference(ident)
    with open(path, "w") as fh:
        fh.write("".join(f">{rid} planted\n{seq}\n" for rid, seq in records))


# ---- `--ends --endref` end to end: what the CLI tests (host emulation and GPU) check
def _rows(path):
    import csv
    return list(csv.reader(open(path)))


def check_cli_outputs(outdir, ident, k=4, min_kmers=ec.MIN_KMERS):
    """ref_ends_{k}.csv, named_reads_{k}.csv and named_ends_{k}.csv say what the planted set asks for (fixed in advance): every planted
    read of ends 1 - 5 with a stored boundary and at least min_kmers kept k-mers is named to its own end; no read of end 6 and no
    unrelated read is named; the group of each of ends 1 - 5 carries its end's name with agree = named, the group of end 6 none; the
    files are consistent with each other and with end_reads_{k}.csv.  Returns (the sorted errors of ref_length against the planted
    length + (the reference end's boundary - 2500), the named reads)."""
    import os
    from topsicle_amd import endref
    _reads, truth, _tails, telo = ec.detection_reads(ident)
    _records, ref_truth = detection_reference(ident)
    refs = _rows(os.path.join(outdir, f"ref_ends_{k}.csv"))
    assert refs[0] == endref.REF_HEADER == ["name", "record", "side", "length", "tail", "boundary", "window_begin", "window_end", "kmers", "indexed",
                                            "reads_named", "groups_named"]
    refs = refs[1:]
    assert [r[0] for r in refs] == list(ref_truth) and all(r[0] == f"{r[1]}_{r[2]}" for r in refs)
    for r in refs:                                 # every piece is an end: a boundary near the planted one, the telomere on its own side
        assert r[4] == ("forward" if r[2] == "head" else "reverse") and abs(int(r[5]) - REF_TELO) <= 100 and r[6] == r[5] and r[9] == "1", r
        assert int(r[7]) == int(r[6]) + ec.SPAN and int(r[8]) >= min_kmers
    boundary = {r[0]: int(r[5]) for r in refs}
    e_rows = _rows(os.path.join(outdir, f"end_reads_{k}.csv"))[1:]
    n_rows = _rows(os.path.join(outdir, f"named_reads_{k}.csv"))
    assert n_rows[0] == endref.READ_HEADER == ["file", "readID", "tail", "telo_length", "end", "name", "offset", "votes", "second", "total", "runner_name",
                                               "runner", "ref_length"]
    n_rows = n_rows[1:]
    assert [r[:4] + [r[4]] for r in n_rows] == [r[:4] + [r[7]] for r in e_rows]            # the same reads in the same order, the same groups
    errors, n_named = [], 0
    for r, e in zip(n_rows, e_rows):
        i = int(r[1][4:])
        if int(e[6]) < min_kmers:
            assert r[5:] == [""] * 8
            continue
        assert all(x != "" for x in (r[6], r[7], r[8], r[9], r[11]))                        # placed: the figures are there
        is_named = r[9] != "0" and int(r[7]) >= MIN_VOTES and int(r[7]) >= RATIO * int(r[8])
        assert (r[5] != "") == (r[12] != "") == is_named and (r[10] != "") == (int(r[11]) > 0)
        own = [name for name, t in ref_truth.items() if t == truth[i]]
        if own:
            assert r[5] == own[0], f"{ident}: read {i} of planted end {truth[i]} is named {r[5]!r}"
            assert int(r[12]) == int(r[3]) - int(r[6])
            errors.append(abs(int(r[12]) - (telo[i] + boundary[r[5]] - REF_TELO)))
            n_named += 1
        else:
            assert r[5] == "", f"{ident}: read {i} (planted end {truth[i]}) is named {r[5]}"
    g_rows = _rows(os.path.join(outdir, f"named_ends_{k}.csv"))
    assert g_rows[0] == endref.GROUP_HEADER == ["end", "reads", "named", "name", "agree", "other_names", "ref_min", "ref_median", "ref_mean", "ref_max",
                                                "called_sd", "ref_sd"]
    groups = {}
    for r in n_rows:
        if r[4] != "0":
            groups.setdefault(int(r[4]), []).append(r)
    assert [int(r[0]) for r in g_rows[1:]] == sorted(groups)
    names_seen = []
    for row in g_rows[1:]:
        mem = groups[int(row[0])]
        planted = {truth[int(r[1][4:])] for r in mem}
        assert len(planted) == 1
        nam = [r for r in mem if r[5] != ""]
        assert int(row[1]) == len(mem) and int(row[2]) == len(nam)
        own = [name for name, t in ref_truth.items() if t == next(iter(planted))]
        if not own:
            assert row[2:] == ["0", "", "0", "0"] + [""] * 6                                # end 6: no name
            continue
        assert row[3] == own[0] and row[4] == row[2] and row[5] == "0" and len(nam) >= ec.MIN_READS
        names_seen.append(row[3])
        a = np.array([int(r[12]) for r in nam], np.float64)
        called = np.array([int(r[3]) for r in nam], np.float64)
        assert (int(row[6]), row[7], row[8], int(row[9])) == (int(a.min()), "%.1f" % np.median(a), "%.1f" % a.mean(), int(a.max()))
        assert (row[10], row[11]) == ("%.1f" % np.std(called, ddof=1), "%.1f" % np.std(a, ddof=1))
    assert sorted(names_seen) == sorted(name for name, t in ref_truth.items() if t != DECOY)          # each of ends 1 - 5 has its group
    for r in refs:
        assert int(r[10]) == sum(x[5] == r[0] for x in n_rows) and int(r[11]) == names_seen.count(r[0])
    return sorted(errors), n_named
