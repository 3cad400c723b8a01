"""End groups (tps_batch_end_sketch, tps_sketch_links; csrc/tps_ends.h) on the host emulation of the two kernels: equal to the plain
restatement of the rules (tests/ends_oracle.py) bit for bit on every case of tests/ends_cases.py, the stand-alone sanitizer run of
the same kernel text on the same cases, the library's refusals, the grouping of topsicle_amd.ends, and detection on planted ends."""
import subprocess

import numpy as np
import pytest

import emu_ends_driver as emu
import ends_cases as ec
import ends_oracle as orc
from topsicle_amd import ends, hiplib


@pytest.mark.parametrize("name", ec.CASE_IDS)
def test_emulation_equals_oracle(name):
    c = ec.case(name)
    got = emu.end_sketch(c.reads, c.unit, c.tails, c.begin, c.end, c.k, c.buckets, base_shift=ec.CASE_IDS.index(name) & 3)
    ec.assert_equal(got, name)


def test_cases_reach_what_they_are_for():
    """The edge cases say what they claim to say (on the oracle's answers)."""
    for name in ec.CASE_IDS:
        c = ec.case(name)
        if name.startswith(("mirror_", "k", "buckets", "albicans23_", "AAAC_")):
            sk, kept = ec.expected(name)
            assert sk.shape == (6, c.buckets)
            for i in (0, 2, 4):                    # tail 0 and tail 1 of one molecule
                assert np.array_equal(sk[i], sk[i + 1]) and kept[i] == kept[i + 1]
            assert (kept[::2] > 0).all() and (sk != ec.EMPTY).any(), name
            assert len({sk[i].tobytes() for i in (0, 2, 4)}) == 3                      # different molecules, different rows
    assert {len(ec.case(f"mirror_{k}").unit) for k in ec.UNITS} == {4, 6, 7, 23, 32}
    assert {(ec.case(n).k) for n in ec.CASE_IDS} >= {8, 12, 16} and {(ec.case(n).buckets) for n in ec.CASE_IDS} == {64, 128, 256, 512}
    # the 300 bases of telomere hold (almost) no kept k-mer: far fewer than the window's positions
    sk, kept = ec.expected("telomere_head")
    assert (kept < 300).all() and (kept > 100).all(), kept                             # 489 positions, ~189 of them in the clean stretch
    # seams: every window spans three pieces; the planted words start at every place from piece 1's first position -- the last word piece 0
    # looks at among them -- to the first letter piece 0 does not stage, and over the second cut
    piece, c = emu.piece(), ec.case("seam")
    places, lone = ec.seam_places(piece)
    k, w = c.k, len(c.unit)
    assert all(e - b - k + 1 > 2 * piece for b, e in zip(c.begin, c.end))
    assert min(places[:-1]) == piece and max(places[:-1]) == piece + k - 1 and piece - 1 + k - w in places and places[-1] + w > 2 * piece > places[-1]
    words = orc.repeat_words(c.unit)
    for r, p in enumerate(places):
        h = orc.telomere_first(c.reads[r], c.tails[r])
        b = c.begin[r]
        assert h[b + p:b + p + w] in words
        kept_at = set(orc.kept_positions(h, b, c.end[r], c.unit, k, words))
        assert not any(b + p - d in kept_at for d in range(k - w + 1))                 # every k-mer that holds the word
        # the lone word: the first repeat word around it decides -- the k-mer that ENDS with it is out, the one before is in
        p0 = min(q for q in range(b + lone - k, b + lone + 1) if h[q:q + w] in words)
        assert p0 - (k - w) not in kept_at and p0 - (k - w) - 1 in kept_at
    sk, kept = ec.expected("letters")
    assert kept[1] < kept[0] and kept[2] == kept[0] and np.array_equal(sk[2], sk[0]) and kept[3] == kept[1] and kept[4] == 0
    assert np.array_equal(sk[:5], sk[5:]) and np.array_equal(kept[:5], kept[5:])
    for k in (8, 12, 16):
        sk, kept = ec.expected(f"bounds_k{k}")
        assert kept.tolist() == [500 - k + 1, 500 - k + 1, 0, 0, 1, 1, 0, 0] * 2 + [0, 0]
        assert np.array_equal(sk[0], sk[1]) and (sk[[2, 3, 6, 7, 16, 17]] == ec.EMPTY).all() and (sk[4] != ec.EMPTY).sum() == 1
    c = ec.case("longest")
    assert c.end[0] - c.begin[0] == hiplib.ENDS_MAX_WINDOW == 16384
    sk, kept = ec.expected("longest")
    assert kept[0] == kept[1] > 8000 and np.array_equal(sk[0], sk[1]) and kept[2] > 4000
    assert ec.expected("empty")[0].shape == (0, 256)


def test_hash_is_murmur3s_finaliser():
    """Known values of fmix32 (MurmurHash3's test vectors for the 32-bit finaliser) and one k-mer by hand."""
    assert orc.fmix32(0) == 0 and orc.fmix32(1) == 0x514E28B7 and orc.fmix32(0xFFFFFFFF) == 0x81F16F39
    assert orc.kmer_hash("ACGTACGTACGT") == orc.fmix32((sum(c << (2 * q) for q, c in enumerate([0, 1, 3, 2] * 3))) ^ 0x9E3779B9)
    sk, kept = emu.end_sketch(["ACGTACGTACGT"], "CCCTAA", [0], [0], [12])
    x = orc.kmer_hash("ACGTACGTACGT")
    assert kept[0] == 1 and sk[0, x >> 24] == x and (sk[0] != ec.EMPTY).sum() == 1


@pytest.mark.parametrize("name", ec.LINK_IDS)
def test_links_equal_oracle(name):
    s, mm, ml = ec.link_sets()[name]
    ec.assert_links_equal(emu.sketch_links(s, mm, ml), ec.expected_links(name), name)


def test_links_on_planted_groups_equal_oracle():
    """600 random sketches with 12 planted groups of 10 (the GPU test takes 1500 with 30): degrees over max_links among them."""
    s = ec.planted_sketches(600, 12)
    want = orc.sketch_links(s, 6, 4)
    ec.assert_links_equal(emu.sketch_links(s, 6, 4), want, "planted")
    assert want[0].sum() == 12 * 45 and (want[0] > 4).any() and (want[0][120:] == 0).all()


def test_link_sets_reach_what_they_are_for():
    degree, links, matches = ec.expected_links("ties")
    assert degree.tolist() == [2, 0, 1, 0, 0, 0] and links[0].tolist() == [2, 3, -1, -1] and matches[0].tolist() == [6, 7, 0, 0]          # 5 is no link, 6 is
    assert links[2, 0] == 3 and matches[2, 0] == 6                                      # rows 2 and 3 share the first 6 through row 0
    assert ec.expected_links("all_empty")[0].tolist() == [0] * 5
    degree, links, _ = ec.expected_links("overflow")
    assert degree[0] == 9 and degree[1] == 8 and links[0].tolist() == [1, 3, 4, 6] and links[1].tolist() == [3, 4, 6, 7]
    assert ec.expected_links("overflow_1")[1][:2, 0].tolist() == [1, 3]
    degree, links, _ = ec.expected_links("n1")
    assert degree.tolist() == [0] and (links == -1).all()
    degree, links, matches = ec.expected_links("n65")
    assert links[0, 0] == 64 and matches[0, 0] == 8 and links[10, :2].tolist() == [30, 64] and links[30, 0] == 64
    assert links[2, 0] == 63 and links[40, 0] == 63 and degree.sum() == 6
    assert ec.expected_links("n65_cut")[1].shape == (65, 3)
    degree, _, _ = ec.expected_links("b512_n130")
    assert degree[0] == 42 and degree[5] == 3


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("ends_cases") / "cases.txt"
    with open(path, "w") as fh:
        for c in ec.cases():
            fh.write(f"case {c.unit} {c.k} {c.buckets} {len(c.reads)}\n")
            fh.write("".join(f"{t} {b} {e} {r or '-'}\n" for r, t, b, e in zip(c.reads, c.tails, c.begin, c.end)))
    return str(path)


def test_standalone_program_is_clean_under_sanitizers(cases_file):
    """The same kernel text under -fsanitize=address,undefined, as a program of its own, on the cases of this file: poisoned LDS of
    exactly one wave's size, a table and a bucket-major copy of exactly their sizes, garbage around the batch; every sketch and every
    link row checked against the program's own restatement of the rules.  Then its built-in batch."""
    exe = emu.build_main()
    for argv in ([exe, cases_file], [exe]):
        out = subprocess.run(argv, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert out.stdout.startswith("ok 4 cases")


@pytest.mark.parametrize("kw, code", ec.SKETCH_REFUSALS)
def test_sketch_refusals_carry_the_librarys_codes(kw, code):
    """TPS_E_ARG (-3) and TPS_E_CAPACITY (-5) as tps_batch_end_sketch returns them (test_gpu_ends.py asks the library the same)."""
    a = dict(code=ec.U6, m=6, tails=[0], begin=[0], end=[100], k=12, buckets=256, lens=None)
    emu.end_sketch_code(["ACGT" * 30], **a)
    emu.end_sketch_code(["ACGT" * 30], **dict(a, end=[16384]))                          # the longest window is taken
    a.update(kw)
    with pytest.raises(hiplib.TopsicleHipError) as e:
        emu.end_sketch_code(["ACGT" * 30], **a)
    assert code in str(e.value)


@pytest.mark.parametrize("kw, code", ec.LINK_REFUSALS)
def test_link_refusals_carry_the_librarys_codes(kw, code):
    s = np.arange(128, dtype=np.uint32).reshape(2, 64)
    a = dict(min_match=6, max_links=4, buckets=None, lens=None, n=None)
    emu.sketch_links(s, **a)
    a.update(kw)
    with pytest.raises(hiplib.TopsicleHipError) as e:
        emu.sketch_links(s, **a)
    assert code in str(e.value)


def test_grouping_equals_the_oracles():
    """topsicle_amd.ends.group (union-find) against the oracle's components: numbering by size, ties to the earlier first member,
    small components unassigned; edge_stats counts both directions."""
    links = np.full((12, 3), -1, np.int32)
    matches = np.zeros((12, 3), np.int32)
    for i, j, m in ((0, 5, 9), (5, 7, 6), (1, 2, 8), (2, 3, 7), (1, 3, 30), (4, 6, 6), (8, 9, 10), (9, 10, 11), (10, 11, 6)):
        p = int((links[i] >= 0).sum())
        links[i, p], matches[i, p] = j, m
    edges = [(i, int(j)) for i in range(12) for j in links[i] if j >= 0]
    for min_reads in (1, 2, 3, 4, 5):
        assert ends.group(12, links, min_reads).tolist() == orc.groups(12, edges, min_reads)
    assert ends.group(12, links, 3).tolist() == [2, 3, 3, 3, 0, 2, 0, 2, 1, 1, 1, 1]          # {8..11} first, then {0,5,7} before {1,2,3}
    n_edges, best = ends.edge_stats(12, links, matches)
    assert n_edges.tolist() == [1, 2, 2, 2, 1, 2, 1, 1, 1, 2, 2, 1] and best.tolist() == [9, 30, 8, 30, 6, 9, 6, 6, 10, 11, 11, 6]
    assert ends.group(0, np.zeros((0, 4), np.int32)).tolist() == []
    assert ends.check("CCCTAA") is None and ends.check("CCT") is not None and ends.check("CCCTAA", k=7) is not None
    assert ends.check("CCCTAA", buckets=100) is not None and ends.check("CCCTAA", min_match=257) is not None and ends.check("CCCTAA", span=16385) is not None


@pytest.mark.parametrize("ident", ec.DETECT_IDS)
def test_planted_ends_are_found(ident):
    """6 planted ends x 12 reads and 20 unrelated reads, the defaults, windows at the planted boundary +- 300.  Fixed in advance: no
    group holds reads of two planted ends, no unrelated read is assigned.  The kernel path (emulation) equals the oracle exactly --
    sketches, links and groups -- and the oracle alone puts at least 90 % of the planted reads into their end's one group (the
    share is in the README)."""
    reads, truth, tails, _telo = ec.detection_reads(ident)
    begin, end = ec.detection_windows(ident)
    motif = ident.rsplit("_", 1)[0]
    want = orc.end_sketch(reads, motif, tails, begin, end, ec.K, ec.BUCKETS)
    got = emu.end_sketch(reads, motif, tails, begin, end, ec.K, ec.BUCKETS)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    g_end, g_deg = ec.groups_from(got[0], got[1], emu.sketch_links)
    w_end, w_deg = ec.groups_from(want[0], want[1], orc.sketch_links)
    assert g_end == w_end and np.array_equal(g_deg, w_deg)
    part = [i for i in range(len(reads)) if got[1][i] >= ec.MIN_KMERS]
    assert ends.group(len(part), emu.sketch_links(got[0][part], ec.MIN_MATCH, ec.MAX_LINKS)[1], ec.MIN_READS).tolist() == [g_end[i] for i in part]
    for g in set(g_end) - {0}:
        assert len({truth[i] for i in range(len(reads)) if g_end[i] == g}) == 1, f"group {g} mixes planted ends"
    assert all(g_end[i] == 0 for i in range(len(reads)) if truth[i] == 0), "an unrelated read was assigned"
    # the share: a planted read counts when it is in the largest group of its end
    good = 0
    for e in range(1, ec.N_ENDS + 1):
        mine = [w_end[i] for i in range(len(reads)) if truth[i] == e and w_end[i]]
        good += max((mine.count(g) for g in set(mine)), default=0)
    print(f"{ident}: the oracle assigns {good} of {ec.N_ENDS * ec.PER_END} planted reads to their end's group")
    assert good >= 0.9 * ec.N_ENDS * ec.PER_END
