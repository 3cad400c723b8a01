"""Anchored lengths (tps_batch_end_window, tps_window_offsets; csrc/tps_anchor.h) on the host emulation of the two kernels: equal to
the plain restatement of the rules (tests/anchor_oracle.py) bit for bit on every case of tests/anchor_cases.py, popcount(keep) equal
to the sketch's kept, the stand-alone sanitizer run of the same kernel text on the same cases, the library's refusals, the host rule
of topsicle_amd.anchor, and the detection claim on the planted ends."""
import subprocess

import numpy as np
import pytest

import anchor_cases as ac
import anchor_oracle as orc
import emu_anchor_driver as emu
import emu_ends_driver
import ends_cases as ec
import ends_oracle as eo
from topsicle_amd import anchor, hiplib


@pytest.mark.parametrize("name", ac.WINDOW_IDS)
def test_window_emulation_equals_oracle(name):
    c = ac.case(name)
    got = emu.end_window(c.reads, c.unit, c.tails, c.begin, c.end, c.k, c.span, base_shift=ac.CASE_IDS.index(name) & 3)
    ac.assert_rows_equal(got, name)


@pytest.mark.parametrize("name", ac.CASE_IDS)
def test_offset_emulation_equals_oracle(name):
    c, want = ac.case(name), ac.expected(name)
    ac.assert_offsets_equal(emu.window_offsets(want["codes"], want["keep"], want["length"], c.ref, c.span, c.k), name)


@pytest.mark.parametrize("name", ac.WINDOW_IDS)
def test_keep_bits_count_what_the_sketch_keeps(name):
    """popcount(keep[r]) == kept[r] of the sketch of the same window: on the emulations of both kernels and on both oracles."""
    c = ac.case(name)
    if not c.reads:
        return
    _codes, keep = emu.end_window(c.reads, c.unit, c.tails, c.begin, c.end, c.k, c.span)
    _sk, kept = emu_ends_driver.end_sketch(c.reads, c.unit, c.tails, c.begin, c.end, c.k, 64)
    assert np.array_equal(ac.popcount(keep), kept)
    assert np.array_equal(ac.popcount(ac.expected(name)["keep"]), eo.end_sketch(c.reads, c.unit, c.tails, c.begin, c.end, c.k, 64)[1])


def test_cases_reach_what_they_are_for():
    """The edge cases say what they claim to say (on the oracle's answers)."""
    c, w = ac.case("lengths"), ac.expected("lengths")
    assert w["length"].tolist() == list(ac.LENGTHS) * 2 and c.span == hiplib.ANCHOR_MAX_SPAN == 4096 and set(c.tails) == {0, 1}
    assert np.array_equal(w["codes"][:11], w["codes"][11:]) and np.array_equal(w["keep"][:11], w["keep"][11:])           # tail 1 = tail 0
    assert (w["keep"][:, 0] & 0xFF == 0).all() and not any(min(s, default=99) < 9 for s in w["keeps"])                      # begun inside the repeat
    assert (w["keep"][:3] == 0).all() and (w["codes"][0] == 0).all() and (w["codes"][1] != 0).any()                         # 0, k - 1, k letters
    big = w["keeps"][10]
    assert not any(q in big for q in list(range(3958, 3965)) + list(range(3969, 3976)))                                      # the words over the seam of the two pieces
    assert max(big) > 4000 and sum(q >= 3968 for q in big) > 30 and len(big) > 2000
    offset, votes, second = w["offsets"]
    assert (offset == 0).all() and votes[0] == votes[1] == votes[2] == 0 and votes[3] > 0 and votes[10] > 2000 and votes[10] == votes[21]
    w = ac.expected("past_end")
    assert w["length"].tolist() == [400, 437, 300, 0, 11, 0] * 2 + [0]
    assert w["offsets"][0][:3].tolist() == [0, -37, 100] and w["offsets"][1][3:6].tolist() == [0, 0, 0]
    w = ac.expected("letters")
    kp = ac.popcount(w["keep"])
    assert kp[1] < kp[0] and kp[2] == kp[0] and kp[4] == 0 and (w["codes"][4] == 0).all() and np.array_equal(w["codes"][:5], w["codes"][5:])
    assert w["offsets"][0][3] == 10 and w["offsets"][1][4] == 0
    for key in ac.UNITS:
        offset, votes, second = ac.expected(f"unit_{key}")["offsets"]
        assert offset.tolist() == [0, 37, 0, 0, 37, 0, 0, 37, -100] and votes[5] <= 1 and votes[2] == 0 and (votes[[0, 1, 3, 4, 6, 7, 8]] > 100).all()
    assert {ac.case(n).k for n in ac.CASE_IDS} >= {8, 12, 16} and {ac.case(n).span for n in ac.CASE_IDS} >= {12, 33, 65, 1999, 2000, 2001, 4096}
    offset, votes, second = ac.expected("table")["offsets"]
    assert (offset[1], votes[1]) == (50, 1) and (offset[2], votes[2]) == (45, 1)                                            # the smaller q of a duplicated k-mer
    assert votes[[4, 5, 7, 8]].tolist() == [1, 0, 1, 0] and (offset[4], offset[7]) == (-4, 8) and (offset[10], votes[10]) == (-4, 1)
    assert votes[11] <= 1 and votes[12:].tolist() == [0, 0, 0] and votes[3] == 0 and second[0] >= 1
    offset, votes, second = ac.expected("bin_edges")["offsets"]
    assert offset.tolist() == [0, 64, 63, 128, 127, 1, -64, -65, -63, -1, 63, 128] and (votes > 100).all() and second[:11].max() <= 2 and second[11] > 100
    for k in (8, 12, 16):
        offset, votes, second = ac.expected(f"extreme_k{k}")["offsets"]
        assert offset.tolist() == [-(4096 - k), 4096 - k] and votes.tolist() == [1, 1]
    offset, votes, second = ac.expected("median")["offsets"]
    assert (offset[1], votes[1], second[1]) == (40, 30, 30) and (offset[2], votes[2], second[2]) == (500, 31, 30)          # equal maxima: the smaller c
    assert offset[3:].tolist() == [98, 98, 98, 100] and votes[3:].tolist() == [2, 4, 6, 5]                                   # the lower median
    assert max(len(c.ref) for c in ac.cases()) <= 40


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("anchor_cases") / "cases.txt"
    with open(path, "w") as fh:
        for c in ac.cases():
            if c.by_hand:
                fh.write(f"ocase {c.k} {c.span} {len(c.windows)}\n")
                for win, kept, ref in zip(c.windows, c.keeps, c.ref):
                    fh.write(f"{ref} {win or '-'} {''.join('1' if q in kept else '0' for q in range(len(win))) or '-'}\n")
            else:
                fh.write(f"wcase {c.unit} {c.k} {c.span} {len(c.reads)}\n")
                fh.write("".join(f"{t} {b} {e} {ref} {r or '-'}\n" for r, t, b, e, ref in zip(c.reads, c.tails, c.begin, c.end, c.ref)))
    return str(path)


def test_standalone_program_is_clean_under_sanitizers(cases_file):
    """The same kernel text under -fsanitize=address,undefined, as a program of its own, on the cases of this file: poisoned LDS of
    exactly one wave's size, rows and tables of exactly their sizes, garbage around the batch; every window and every offset checked
    against the program's own restatement of the rules.  Then its built-in batch."""
    exe = emu.build_main()
    for argv in ([exe, cases_file], [exe]):
        out = subprocess.run(argv, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert out.stdout.startswith("ok 4 cases")


@pytest.mark.parametrize("kw, code", ac.WINDOW_REFUSALS)
def test_window_refusals_carry_the_librarys_codes(kw, code):
    """TPS_E_ARG (-3) and TPS_E_CAPACITY (-5) as tps_batch_end_window returns them (test_gpu_ends_anchor.py asks the library the same)."""
    a = dict(ac.WINDOW_GOOD)
    emu.end_window_code(["ACGT" * 30], **a)
    a.update(kw)
    with pytest.raises(hiplib.TopsicleHipError) as e:
        emu.end_window_code(["ACGT" * 30], **a)
    assert code in str(e.value)


@pytest.mark.parametrize("kw, code", ac.OFFSET_REFUSALS)
def test_offset_refusals_carry_the_librarys_codes(kw, code):
    codes, keep = np.zeros((2, 7), np.uint32), np.zeros((2, 4), np.uint32)
    a = dict(ac.OFFSET_GOOD)
    assert [x.tolist() for x in emu.window_offsets(codes, keep, **a)] == [[0, 0]] * 3
    a.update(kw)
    with pytest.raises(hiplib.TopsicleHipError) as e:
        emu.window_offsets(codes, keep, **a)
    assert code in str(e.value)


def test_host_rule_equals_the_oracles():
    """topsicle_amd.anchor (numpy) against the oracle's lists: the reference of a group, the anchoring test, the consensus, the shift."""
    end = [1, 2, 1, 0, 2, 1, 2, 3, 3]
    links = [2, 5, 3, 9, 5, 3, 1, 0, 0]
    ref = anchor.references(end, links)
    assert ref.tolist() == orc.references(end, links) == [2, 1, 2, -1, 1, 2, 1, 7, 7]          # the most links, ties to the first
    begin = [1000, 2000, 1100, 500, 2100, 900, 2050, 700, 800]
    telo = list(begin)
    offset = [90, 0, 0, 0, 120, -200, 40, 0, 3]
    votes = [300, 900, 800, 999, 20, 19, 40, 21, 50]
    second = [3, 0, 0, 0, 5, 0, 11, 5, 13]
    anchored, pos, cons = anchor.anchor_groups(end, ref, begin, offset, votes, second)
    want_reads, want_cons = orc.anchor(end, ref, begin, telo, offset, votes, second)
    assert anchored.tolist() == [w is not None for w in want_reads] == [True, True, True, False, True, False, False, True, False]
    assert cons == {g: c for g, c in want_cons.items() if c is not None} == {1: 1100, 2: 2000, 3: 700}
    assert [int(cons[end[i]] - pos[i]) for i in range(9) if anchored[i]] == [w[0] for w in want_reads if w is not None] == [-90, 0, 0, -120, 0]
    assert anchor.check(False, 2000) is not None and anchor.check(True, 4097) is not None and anchor.check(True, 4096) is None
    assert anchor.check(True, 2000, 0, 4) is not None


@pytest.mark.parametrize("ident", ec.DETECT_IDS)
def test_planted_reads_are_anchored(ident):
    """6 planted ends x 12 reads and 20 unrelated reads, windows at the planted boundary +- 300, groups and references by the host
    rule, the defaults.  Fixed in advance: every planted read is anchored; no unrelated read forced against a reference reaches
    anchorminvotes; the pairwise error of anchored differences against planted differences within an end has p95 <= 40 and max <= 80
    (ONT), p95 <= 10 and max <= 20 (HiFi).  The kernel path (emulation) equals the oracle exactly, so the figures are the rule's."""
    reads, truth, tails, telo = ec.detection_reads(ident)
    rows = ac.detection_rows(ident)
    g_end, n_links = ac.detection_groups(ident)
    motif = ident.rsplit("_", 1)[0]
    begin, end = ec.detection_windows(ident)
    codes, keep = emu.end_window(reads, motif, tails, begin, end, ec.K, ec.SPAN)
    assert np.array_equal(codes, rows["codes"]) and np.array_equal(keep, rows["keep"])
    ref = anchor.references(g_end, n_links)
    assert ref.tolist() == rows["ref"]
    want = orc.window_offsets(rows["windows"], rows["keeps"], rows["ref"], ec.K)
    got = emu.window_offsets(codes, keep, rows["length"], ref, ec.SPAN, ec.K)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    anchored_err, called_err = ac.detection_errors(ident, g_end, rows["ref"], begin, *got)
    a_anchored, _pos, _cons = anchor.anchor_groups(g_end, ref, begin, *got)
    assert a_anchored.tolist() == [t != 0 for t in truth]
    grouped = [i for i in range(len(reads)) if g_end[i]]
    # unrelated reads forced against every group's reference
    lone = [i for i in range(len(reads)) if truth[i] == 0]
    refs = sorted(set(rows["ref"]) - {-1})
    idx = refs + lone * len(refs)
    forced = list(range(len(refs))) + [r for r in range(len(refs)) for _ in lone]
    f_off, f_votes, f_second = emu.window_offsets(codes[idx], keep[idx], rows["length"][idx], forced, ec.SPAN, ec.K)
    w_votes = orc.window_offsets([rows["windows"][i] for i in idx], [rows["keeps"][i] for i in idx], forced, ec.K)[1]
    assert np.array_equal(f_votes, w_votes)
    p95, worst = ac.BOUNDS[ident.rsplit("_", 1)[1]]
    print(f"{ident}: anchored differences median / p95 / max {np.median(anchored_err):.0f} / {np.percentile(anchored_err, 95):.0f} / {anchored_err[-1]}, "
          f"called boundaries {np.median(called_err):.0f} / {np.percentile(called_err, 95):.0f} / {called_err[-1]}; votes of a planted read >= {got[1][grouped].min()}, "
          f"runner-up <= {got[2][grouped].max()}, an unrelated read <= {f_votes[len(refs):].max()}")
    assert f_votes[len(refs):].max() < ac.MIN_VOTES
    assert np.percentile(anchored_err, 95) <= p95 and anchored_err[-1] <= worst
