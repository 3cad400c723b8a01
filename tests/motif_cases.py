"""Test helper: the reads and parameter sets of the motif census tests (tests/test_motif_census.py on the host emulation,
tests/test_gpu_motif.py on the GPU), and the oracle's answers to them, computed once per process (tests/motif_oracle.py)."""
import functools

import numpy as np

import motif_oracle
from topsicle_amd import hiplib, synth

M32 = "ACGGTTCAGTCCATGACTTGCAAGTCTGATCC"           # 32 letters, no shorter period
assert len(M32) == 32

MOTIFS = {                                         # the sets the vote is checked on (tally): name -> motif
    "CCCTAA": "CCCTAA",
    "AAACCCT": "AAACCCT",
    "CCCTAAAA": "CCCTAAAA",
    "glabrata16": "CTGTGGGGTCTGGGTG",              # C. glabrata, 16 letters
    "albicans23": "ACGGATGTCTAACTTCTTGGTGT",       # C. albicans, 23 letters
    "lactis25": "ACGGATTTGATTAGGTATGTGGTGT",       # K. lactis, 25 letters
}
assert [len(m) for m in MOTIFS.values()] == [6, 7, 8, 16, 23, 25]


def vote_reads(name, errors):
    """The 200 reads of 6000 bases the support floor was chosen on: half of them telomeric, tracts of 300 to 3000 bases."""
    b, o, _ = synth.make_reads(200, 6000, MOTIFS[name], seed=5, errors=errors, tract_min=300, tract_max=3000, telomeric_fraction=0.5)
    return synth.split_reads(b, o)


@functools.lru_cache(maxsize=None)
def pool():
    """One batch of reads with everything the rule has a case for."""
    rng = np.random.default_rng(11)
    rnd = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))      # noqa: E731
    b, o, _ = synth.make_reads(6, 6000, "CCCTAA", seed=3, tract_min=300, tract_max=3000, telomeric_fraction=0.7)
    reads = synth.split_reads(b, o)
    reads += [
        "CCCTAA" * 1000,                                   # a perfect tract over the whole span
        M32 * 150,                                         # all 64 bits of the unit
        "A" * 5000,                                        # every period ties: u_min wins, one run across every word boundary
        "T" * 33,
        "c" * 100 + "g" * 100,
        ("ccctaa" * 200 + rnd(500)).lower(),               # lower case
        "CCCTAAA" * 40 + "N" + "CCCTAAA" * 40 + "RYK" + "CCCTAAA" * 60 + rnd(700),      # N / IUPAC next to and inside runs
        "N" * 50 + "CCCTAA" * 30 + "N" + "CCCTAA" * 3 + "n" + rnd(300) + "N" * 20,
        "ACGTACGTAC" + "N" + "GTACGTACGTACGT" * 10,
        M32[:20] + "N" + M32[21:] + M32[:19],              # the only run starts at 0: an N behind the first 8 letters of the 32-letter unit
        "N" * 300,
        rnd(700),                                          # shorter than hi: both ends overlap
        "CCCTAA" * 60 + rnd(100) + "TTAGGG" * 60,          # 820 bases, a tract at either end
        "", "A", "AC", "ACG",
    ]
    reads += [("CCCTAA" * 30)[:n] for n in (11, 12, 15, 16, 17, 19, 20, 31, 32, 33, 39, 40, 47, 48, 49, 63, 64, 65, 127, 128, 129)]
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def ragged():
    """300 ragged reads of 1 .. 6000 bases with N and lower-case reads among them."""
    b, o, _ = synth.make_ragged_reads(300, "CCCTAA", seed=9, len_mu=6.0, len_sigma=2.0, min_len=1, max_len=6000, n_frac=0.01, lower_frac=0.2,
                                      tract_min=300, tract_max=3000, telomeric_fraction=0.6)
    reads = synth.split_reads(b, o)
    assert min(map(len, reads)) == 1 and max(map(len, reads)) == 6000
    return tuple(reads)


# (name, reads, keyword arguments of motif_census)
def cases():
    out = [("defaults", pool(), {}),
           ("ragged", ragged(), {}),
           ("ragged_lo", ragged(), dict(lo=37, hi=2000, u_min=1, u_max=32, min_len=100))]
    # n = u + w - 1 (no position can count) and n = u + w (exactly one can), for w = u and for w = 8
    for u in (1, 6, 12, 32):
        w = min(u, 8)
        out += [(f"n_eq_u{u}_w_minus1", pool(), dict(u_min=u, u_max=u, lo=0, hi=u + w - 1)),
                (f"n_eq_u{u}_w", pool(), dict(u_min=u, u_max=u, lo=0, hi=u + w)),
                (f"n_eq_u{u}_w_lo", pool(), dict(u_min=u, u_max=u, lo=5, hi=5 + u + w))]
    # n a multiple of 16 / 32 and one off either side
    for n in (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025):
        out.append((f"n{n}", pool(), dict(lo=0, hi=n, u_min=1, u_max=32)))
        out.append((f"n{n}_lo61", pool(), dict(lo=61, hi=61 + n)))
    out += [("span4096", pool(), dict(lo=0, hi=4096)),
            ("span4096_lo7", pool(), dict(lo=7, hi=4103, u_min=1, u_max=32)),
            ("span1", pool(), dict(lo=10, hi=11, u_min=1, u_max=4)),
            ("u32_only", pool(), dict(u_min=32, u_max=32, hi=2000)),
            ("u1_only", pool(), dict(u_min=1, u_max=1)),
            ("u1_to_32", pool(), dict(u_min=1, u_max=32)),
            ("min_len", pool(), dict(min_len=820)),          # the 820-base read is left out, 821 would be in
            ("min_len_all", pool(), dict(min_len=6000)),
            ("empty", (), {})]
    return out


CASE_IDS = [c[0] for c in cases()]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(hits, counts) of the oracle for case `name`."""
    _, reads, kw = next(c for c in cases() if c[0] == name)
    return motif_oracle.motif_census(list(reads), want_counts=True, **kw)


def assert_equal(got_hits, got_counts, name, with_counts=True):
    want_hits, want_counts = expected(name)
    assert got_hits.dtype == hiplib.MOTIF_HIT_DTYPE and got_hits.shape == want_hits.shape
    for f in hiplib.MOTIF_HIT_DTYPE.names:
        bad = np.argwhere(got_hits[f] != want_hits[f])
        assert len(bad) == 0, f"{name}: {f} differs at (read, end) {bad[:5].tolist()}: got {got_hits[tuple(bad[0])]}, want {want_hits[tuple(bad[0])]}"
    if with_counts:
        assert got_counts.shape == want_counts.shape
        bad = np.argwhere(got_counts != want_counts)
        assert len(bad) == 0, f"{name}: C_u differs at (read, end, period index) {bad[:5].tolist()}"
    else:
        assert got_counts is None


# ---- the refusals: (what differs from a good call, the return code in the message)
REFUSALS = [
    (dict(u_min=0), "rc=-3"), (dict(u_min=5, u_max=4), "rc=-3"), (dict(u_max=33), "rc=-3"),
    (dict(lo=-1), "rc=-5"), (dict(lo=10, hi=10), "rc=-5"), (dict(lo=0, hi=4097), "rc=-5"),
]
