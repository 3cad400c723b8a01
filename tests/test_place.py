"""Named ends (tps_window_place; csrc/tps_place.h) on the host emulation of the kernel: equal to the plain restatement of the rule
(tests/place_oracle.py) bit for bit on every case of tests/place_cases.py, the stand-alone sanitizer run of the same kernel text on
the same cases, the library's refusals, the host rule of topsicle_amd.endref, and the detection claim on the planted ends."""
import subprocess

import numpy as np
import pytest

import anchor_cases as ac
import emu_place_driver as emu
import ends_cases as ec
import place_cases as pc
import place_oracle as po
from topsicle_amd import endref, hiplib


@pytest.mark.parametrize("name", pc.CASE_IDS)
def test_emulation_equals_oracle(name):
    pc.assert_equal(pc.run_case(emu.place_windows, name), pc.expected(name), name)


def test_cases_reach_what_they_are_for():
    """The edge cases say what they claim to say (on the oracle's answers)."""
    ref, total, runner_ref, runner, offset, votes, second = pc.expected("lengths")
    assert [len(w) for w in pc.case("lengths").windows] == list(pc.LENGTHS) == [0, 11, 12, 75, 76, 77, 4096]
    assert ref.tolist() == [-1, -1, 1, 1, 1, 1, 1] and total.tolist() == votes.tolist() == [0, 0, 1, 64, 65, 66, 4085] and (offset == 0).all()
    assert (runner_ref == -1).all() and (runner == 0).all()                                  # a query equal to its reference: every k-mer votes
    ref, total, *_ = pc.expected("empty_refs")
    assert ref.tolist() == [-1, 3, 3, -1] and total[1] == 189
    assert [x.tolist() for x in pc.expected("single")] == [[0], [139], [-1], [0], [-7], [139], [0]]
    c = pc.case("many_refs")
    assert len(c.ref_windows) == hiplib.PLACE_MAX_REFS == 1024 and len(c.windows) == 13
    ref, total, runner_ref, runner, *_ = pc.expected("many_refs")
    assert ref[:11].tolist() == [0, 1023, 1, 63, 64, 65, 512, 1022, 0, 700, 5] and (runner_ref[8], runner[8]) == (1023, 5) and (ref[10], runner_ref[10]) == (5, 6)
    assert (ref[12], total[12]) == (1023, 1)
    for max_occ in (1, 2, 16):
        ref, total, runner_ref, runner, offset, votes, second = pc.expected(f"occ{max_occ}")
        assert (ref[0], total[0]) == (0, min(max_occ, 2)) and (ref[1], total[1]) == (-1, 0)        # exactly max_occ entries vote, max_occ + 1 are dropped
        assert ref[3] == max_occ and ref[4] == 0
    ref, total, runner_ref, runner, *_ = pc.expected("occ16")
    assert (runner_ref[0], runner[0]) == (1, 1)                                             # 15 rows hold the k-mer once each: the smallest of the equal runner-ups
    ref, total, runner_ref, runner, offset, votes, second = pc.expected("ties")
    assert (ref[0], runner_ref[0], total[0], runner[0]) == (1, 2, 29, 29)                  # equal totals: the smaller row
    assert (ref[1], runner_ref[1], runner[1]) == (3, 1, 29) and (ref[2], runner_ref[2], runner[2]) == (2, -1, 0)
    assert (ref[4], votes[4], second[4], offset[4], total[4]) == (0, 29, 12, 0, 41)              # d = 0 and, two coarse bins away, d = 140 (three letters of the seam fit by chance)
    for k in (8, 12, 16):
        ref, total, _rr, _r, offset, votes, _s = pc.expected(f"extreme_k{k}")
        assert ref.tolist() == [0, 1] and offset.tolist() == [-(4096 - k), 4096 - k] and votes.tolist() == [1, 1]
    ref, total, runner_ref, runner, offset, votes, second = pc.expected("buckets")
    assert ref[:6].tolist() == [1, -1, 1, 1, 1, 1] and total[:6].tolist() == [1, 0, 1, 1, 1, 4] and runner_ref[:6].tolist() == [2, -1, -1, 2, -1, 2]
    for name in ("reads_letters", "reads_unit_CCCTAA"):
        assert (pc.expected(name)[1] > 100).sum() >= 6 and set(ac.case(name[6:]).tails) == {0, 1}
    assert {pc.case(n).k for n in pc.CASE_IDS} >= {8, 12, 16} and {pc.case(n).max_occ for n in pc.CASE_IDS} == {1, 2, 16}
    assert max(len(c.windows) for c in pc.cases()) <= 40


def test_bucket_kmers_lie_where_the_case_says():
    """The directory of the `buckets` case has 12 bits; its hand-picked hashes are in the first bucket, on both sides of the border in
    the middle, and in the last."""
    import ends_oracle as eo
    pc.run_case(emu.place_windows, "buckets")
    bits = emu.dir_bits()
    assert 8 <= bits <= 16
    assert [eo.kmer_hash(s) >> (32 - bits) for s in pc.bucket_kmers()] == [0, 0, (1 << (bits - 1)) - 1, 1 << (bits - 1), (1 << bits) - 1]
    pc.run_case(emu.place_windows, "extreme_k12")
    assert emu.dir_bits() == 4                                                              # (two k-mers: the smallest directory)


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("place_cases") / "cases.txt"

    def line(win, kept):
        return f"{win or '-'} {''.join('1' if q in kept else '0' for q in range(len(win))) or '-'}\n"
    with open(path, "w") as fh:
        for c in pc.cases():
            fh.write(f"pcase {c.k} {c.span} {c.max_occ} {len(c.windows)} {len(c.ref_windows)}\n")
            fh.write("".join(line(w, s) for w, s in zip(c.windows, c.keeps)) + "".join(line(w, s) for w, s in zip(c.ref_windows, c.ref_keeps)))
    return str(path)


def test_standalone_program_is_clean_under_sanitizers(cases_file):
    """The same kernel text under -fsanitize=address,undefined, as a program of its own, on the cases of this file: poisoned LDS of
    exactly one wave's size, rows and an index of exactly their sizes; every output checked against the program's own restatement of
    the rule.  Then its built-in batch."""
    exe = emu.build_main()
    for argv in ([exe, cases_file], [exe]):
        out = subprocess.run(argv, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert out.stdout.startswith("ok 3 cases")


@pytest.mark.parametrize("kw, code", pc.REFUSALS)
def test_refusals_carry_the_librarys_codes(kw, code):
    """TPS_E_ARG (-3) and TPS_E_CAPACITY (-5) as tps_window_place returns them (test_gpu_place.py asks the library the same); the call
    with that one argument corrected succeeds."""
    a = dict(pc.GOOD)
    assert [x.tolist() for x in emu.place_windows(**pc.REFUSAL_ROWS, **a)] == [[-1, -1], [0, 0], [-1, -1], [0, 0], [0, 0], [0, 0], [0, 0]]
    a.update(kw)
    with pytest.raises(hiplib.TopsicleHipError) as e:
        emu.place_windows(**pc.REFUSAL_ROWS, **a)
    assert code in str(e.value)


def test_host_rule_equals_the_oracles():
    """topsicle_amd.endref (numpy) against the oracle's lists: named / not named, the majority name and its ties, ref_length."""
    ref = [0, 2, -1, 1, 1, 2, 0, 2, 1]
    votes = [300, 20, 999, 19, 40, 21, 50, 80, 20]
    second = [3, 5, 0, 0, 11, 5, 13, 20, 6]
    named = endref.named_reads(ref, votes, second)
    assert named.tolist() == po.named(ref, votes, second) == [True, True, False, False, False, True, False, True, False]
    assert endref.named_reads(ref, votes, second, 19, 3).tolist() == po.named(ref, votes, second, 19, 3) == [True, True, False, True, True, True, True, True, True]
    end = [1, 1, 1, 2, 2, 1, 3, 1, 0]
    name_of = [r if n else None for r, n in zip(ref, named)]
    want = po.group_names(end, name_of)
    assert want == {1: (2, 3, [0], 4), 2: (None, 0, [], 0), 3: (None, 0, [], 0)}
    for g, (top, agree, others, n_named) in want.items():
        mine = [name_of[i] for i in range(len(end)) if end[i] == g and name_of[i] is not None]
        assert endref.group_name(mine) == (top, agree, len(others)) and len(mine) == n_named
    assert endref.group_name([3, 1, 3, 1]) == (1, 2, 1) and po.group_names([1] * 4, [3, 1, 3, 1])[1][:2] == (1, 2)        # a tie: the end listed first
    assert endref.check(False, 2000) is not None and endref.check(True, 4097) is not None and endref.check(True, 4096) is None
    assert endref.check(True, 2000, 0) is not None and endref.check(True, 2000, 65) is not None and endref.check(True, 2000, 16, 0) is not None

    class Engine:
        def place_windows(self, codes, keep, length, ref_codes, ref_keep, ref_length, span, k, max_occ):
            assert len(length) == 3 and len(ref_length) == 2 and (span, k, max_occ) == (2000, 12, 16)
            return np.array([[1, 0, -1], [90, 40, 0], [0, -1, -1], [50, 0, 0], [-30, 12, 0], [80, 19, 0], [2, 0, 0]], np.int32)

    row = np.zeros(1, np.uint32)
    rows = [("f", f"read{i}", i & 1, 1000 + i, 1000 + i, 3000 + i, kept, None, 2000, row, row) for i, kept in enumerate((500, 500, 100, 500))]
    read_rows = [[r[0], r[1], "", r[3], 0, 0, r[6], g, 0, 0] for r, g in zip(rows, (1, 1, 1, 0))]
    refs = []
    for j, (name, indexed) in enumerate((("a_head", True), ("a_tail", False), ("b_tail", True))):
        e = endref.RefEnd(name, name[0], name[2:], 9000)
        e.tail, e.boundary, e.begin, e.end, e.kmers, e.usable, e.indexed = j & 1, 2440, 2440, 4440, 900 if indexed else 10, True, indexed
        e.letters, e.codes, e.keep = 2000, row, row
        refs.append(e)
    out_refs, out_reads, out_groups, stats = endref.run(rows, read_rows, refs, Engine(), 12, 2000, 200)
    assert out_reads[0] == ["f", "read0", "forward", 1000, 1, "b_tail", -30, 80, 2, 90, "a_head", 50, 1030]          # ref_length = telo_length - offset
    assert out_reads[1] == ["f", "read1", "reverse", 1001, 1, "", 12, 19, 0, 40, "", 0, ""]                           # placed, 19 votes: no name
    assert out_reads[2] == ["f", "read2", "forward", 1002, 1] + [""] * 8                                            # too few k-mers: not placed
    assert out_reads[3] == ["f", "read3", "reverse", 1003, 0, "", 0, 0, 0, 0, "", 0, ""]
    assert out_groups == [[1, 3, 1, "b_tail", 1, 0, 1030, "1030.0", "1030.0", 1030, "0.0", "0.0"]]
    assert [r[0] for r in out_refs] == ["a_head", "a_tail", "b_tail"] and [r[9:] for r in out_refs] == [[1, 0, 0], [0, 0, 0], [1, 1, 1]]
    assert (stats["listed"], stats["usable"], stats["indexed"], stats["placed"], stats["named"], stats["groups_named"], stats["close"]) == (3, 3, 2, 3, 1, 1, 1)


@pytest.mark.parametrize("ident", ec.DETECT_IDS)
def test_planted_reads_are_named(ident):
    """6 planted ends x 12 reads and 20 unrelated reads, windows at the planted boundary +- 300, against a reference of ends 1 - 5
    (error-free, windows begun at the boundary +- 60) and a decoy that shares half its window with end 1, the defaults.  Fixed in
    advance: every planted read of ends 1 - 5 is named to its own end; no read of end 6 and no unrelated read is named; the error of
    the offset against the planted one has p95 <= 40 and max <= 80 (ONT), p95 <= 10 and max <= 20 (HiFi).  The kernel path (emulation)
    equals the oracle exactly, so the figures are the rule's."""
    import anchor_oracle as orc
    reads, truth, _tails, telo = ec.detection_reads(ident)
    rows = ac.detection_rows(ident)
    motif = ident.rsplit("_", 1)[0]
    subs = pc.detection_subs(ident)
    rng = np.random.default_rng(8000 + ec.DETECT_IDS.index(ident))
    decoy = ec.rand(rng, 500) + subs[0][500:1500] + ec.rand(rng, 3500)
    jitter = [int(rng.integers(-60, 61)) for _ in range(pc.REF_ENDS + 1)]
    ref_mols = [pc.repeats(motif, pc.REF_TELO, e) + s[:5000] for e, s in enumerate(subs[:pc.REF_ENDS] + [decoy])]
    r_begin = [pc.REF_TELO + j for j in jitter]
    r_codes, r_keep, r_windows, r_keeps = orc.end_window(ref_mols, motif, [0] * len(ref_mols), r_begin, [b + ec.SPAN for b in r_begin], ec.K, ec.SPAN)
    r_length = [len(w) for w in r_windows]
    want = po.place_windows(rows["windows"], rows["keeps"], r_windows, r_keeps, ec.K, endref.DEFAULT_MAX_OCC)
    got = emu.place_windows(rows["codes"], rows["keep"], rows["length"], r_codes, r_keep, r_length, ec.SPAN, ec.K, endref.DEFAULT_MAX_OCC)
    pc.assert_equal(got, want, ident)
    ref, total, runner_ref, runner, offset, votes, second = got
    named = endref.named_reads(ref, votes, second)
    own = [i for i, t in enumerate(truth) if 1 <= t <= pc.REF_ENDS]
    rest = [i for i, t in enumerate(truth) if not 1 <= t <= pc.REF_ENDS]
    assert named[own].all() and (ref[own] == np.array(truth)[own] - 1).all() and not named[rest].any()
    # the offset: the read's window begins at rows["begin"], its planted boundary is telo; the reference's at REF_TELO
    err = sorted(abs(int(offset[i]) - ((rows["begin"][i] - telo[i]) - jitter[truth[i] - 1])) for i in own)
    p95, worst = ac.BOUNDS[ident.rsplit("_", 1)[1]]
    print(f"{ident}: offset error median / p95 / max {np.median(err):.0f} / {np.percentile(err, 95):.0f} / {err[-1]}; votes of a planted read >= {votes[own].min()}, "
          f"runner-up diagonals <= {second[own].max()}, votes of a stranger <= {votes[rest].max()}, the decoy's share of the winner's total <= "
          f"{max(runner[i] / total[i] for i in own):.2f}")
    assert votes[rest].max() < pc.MIN_VOTES
    assert np.percentile(err, 95) <= p95 and err[-1] <= worst
