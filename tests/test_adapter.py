"""The adapter search without a GPU (tps_batch_adapter_find; csrc/tps_adapter.h): the kernel's host emulation against the plain
dynamic programme (tests/adapter_oracle.py) on the cases of tests/adapter_cases.py, bit for bit; the emulation as a stand-alone program
under the sanitizers; the refusals; the detection claim on the oracle's answers; and the host rule of topsicle_amd.adapters against its
restatement on plain lists.  tests/test_gpu_adapter.py runs the same cases through the C ABI on the GPU."""
import subprocess

import numpy as np
import pytest

import adapter_cases as ac
import adapter_oracle as orc
import emu_adapter_driver as emu
from topsicle_amd import adapters, hiplib


@pytest.fixture(scope="module", autouse=True)
def built():
    emu.build()


@pytest.mark.parametrize("name", ac.names())
def test_oracle_says_what_the_case_was_built_for(name):
    ac.check_oracle(name)


@pytest.mark.parametrize("name", ac.names())
def test_emulation_equals_oracle(name):
    c = ac.case(name)
    for shift in (0, 3):                           # (the batch at another place inside its buffer: nothing outside a read is looked at)
        ac.assert_equal(emu.adapter_find(list(c.reads), c.patterns, c.tails, c.begin, c.end, base_shift=shift), name)


def test_sanitizer_program_on_every_case(tmp_path):
    """The emulation as a program of its own under -fsanitize=address,undefined: its built-in batch, then every case from a file; each
    answer is checked there against the program's own plain recurrence."""
    prog = emu.build_main()
    out = subprocess.run([prog], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for c in ac.cases():
            f.write(f"acase {len(c.patterns)} {len(c.reads)}\n" + "".join(p + "\n" for p in c.patterns))
            f.write("".join(f"{t} {b} {e} {r or '-'}\n" for r, t, b, e in zip(c.reads, c.tails, c.begin, c.end)))
    out = subprocess.run([prog, str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith(f"ok {len(ac.cases())} cases"), out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def _call(n_pat=1, pat_len=12, code=(0, 0), tail=0, begin=0, end=100, n_reads=None, hits_len=None):
    """One read of 120 letters, n_pat copies of one pattern; what differs from a good call comes as arguments."""
    P = max(n_pat, 0)
    pats = (np.array([code] * max(P, 1), np.uint64), np.array([pat_len] * max(P, 1), np.int32))
    if P == 0:
        pats = (np.zeros((0, 2), np.uint64), np.zeros(0, np.int32))
    lens = (1 if n_reads is None else n_reads, 2 * P if hits_len is None else hits_len)
    return emu.adapter_find(["ACGT" * 30], pats, [tail], [begin], [end], lens=lens)


@pytest.mark.parametrize("kw, code", ac.REFUSALS)
def test_refusals(kw, code):
    """TPS_E_ARG = -3, TPS_E_CAPACITY = -5, as include/topsicle_hip.h lists them; the good call succeeds."""
    with pytest.raises(hiplib.TopsicleHipError) as e:
        _call(**kw)
    assert code in str(e.value)
    assert _call()[0].shape == (1, 1) and _call(end=1024)[0].shape == (1, 1) and _call(n_pat=64)[0].shape == (1, 64)


def test_good_call_answers_are_the_oracles():
    for pat, pl, code in (("A" * 12, 12, (0, 0)), ("G" * 64, 64, ((1 << 64) - 1, (1 << 64) - 1))):
        assert tuple(int(x[0, 0]) for x in _call(pat_len=pl, code=code)) == orc.find(pat, ("ACGT" * 30)[:100])


def test_pattern_codes_and_peq_layout():
    codes, lens = adapters.pattern_codes(["ACGT" * 3, "T" * 33, "G" * 64])
    assert lens.tolist() == [12, 33, 64]
    assert int(codes[0, 0]) == sum(c << (2 * i) for i, c in enumerate([0, 1, 3, 2] * 3)) and int(codes[0, 1]) == 0
    assert int(codes[1, 0]) == int("10" * 32, 2) and int(codes[1, 1]) == 2
    assert int(codes[2, 0]) == (1 << 64) - 1 == int(codes[2, 1])
    with pytest.raises(ValueError):
        adapters.pattern_codes(["ACGTN" * 4])


def test_block_oracle_equals_plain_oracle():
    """The all-at-once restatement the detection sets use, against the plain loop: mixed lengths, N, texts of several lengths."""
    rng = np.random.default_rng(5)
    pats = [ac.rand(rng, m) for m in (12, 31, 64, 24)]
    texts = [ac.rand(rng, n) for n in (0, 1, 30, 100, 257)] + ["ACGNNT" * 20, ac.mutate(rng, pats[2], (0.05, 0.03, 0.03)) + "ACGT"]
    dist, end = orc.find_block(pats, texts)
    for r, t in enumerate(texts):
        for j, p in enumerate(pats):
            assert (int(dist[r, j]), int(end[r, j])) == orc.find(p, t), (r, j)
    ident = "P12_m24_CCCTAA_ONT"
    pats, reads, tails, _planted, _ends = ac.detection_set(ident)
    want = ac.detection_expected(ident)
    for r in range(0, len(reads), 40):
        h = orc.telomere_first(reads[r], tails[r])[:ac.DETECT_SEARCH]
        assert [orc.find(p, h) for p in pats] == [(int(want[0][r, j]), int(want[1][r, j])) for j in range(len(pats))]


@pytest.mark.parametrize("ident", list(ac.SETS))
def test_detection_claim(ident):
    """On the oracle's answers at the defaults (search 256, err 0.2, margin 2): at least 0.97 of the planted reads named, none to a
    wrong pattern, no adapter-free read named, |adapter_end - planted end| <= 4; and the emulation gives the oracle's rows, so the claim
    holds for it."""
    dist, end = ac.detection_expected(ident)
    ac.check_detection(dist, end, ident)
    pats, reads, tails, _planted, _ends = ac.detection_set(ident)
    n = len(reads)
    got = emu.adapter_find(list(reads), list(pats), tails, [0] * n, [ac.DETECT_SEARCH] * n)
    assert np.array_equal(got[0], dist) and np.array_equal(got[1], end)


def test_naming_rule_against_plain_lists():
    rng = np.random.default_rng(11)
    for lens in ([24], [24, 24, 24], [12, 40, 64, 25, 33], [20] * 7):
        P = len(lens)
        dist = rng.integers(0, 12, (300, P))
        dist[:40] = np.minimum(dist[:40], 4)       # rows crowded at small distances: ties of slack, runners inside the margin
        if P > 1:
            dist[40:60, 1] = dist[40:60, 0]        # equal slack (equal lengths) or not (mixed): ties go to the smallest j
        for err, margin in ((0.2, 2), (0.25, 1), (0.1, 0), (0.29, 3)):
            best, runner, named = adapters.name_reads(dist.astype(np.uint16), lens, err, margin)
            for i in range(len(dist)):
                assert (int(best[i]), int(runner[i]), bool(named[i])) == ac.name_rule(dist[i].tolist(), lens, err, margin), (lens, err, margin, i)
    # by hand: thr = floor(0.2 * 24) = 4
    hand = np.array([[4, 9, 9], [5, 9, 9], [2, 3, 9], [2, 4, 9], [3, 3, 9], [9, 9, 1]], np.uint16)
    best, runner, named = adapters.name_reads(hand, [24, 24, 24], 0.2, 2)
    assert best.tolist() == [0, 0, 0, 0, 0, 2] and runner.tolist() == [1, 1, 1, 1, 1, 0]
    assert named.tolist() == [True, False, False, True, False, True]
    assert adapters.name_reads(np.array([[4], [5]], np.uint16), [24], 0.2, 2)[2].tolist() == [True, False]       # P = 1: no margin
    assert adapters.thresholds([12, 24, 28, 40, 64, 100], 0.2).tolist() == [2, 4, 5, 8, 12, 20] and adapters.thresholds([100], 0.29).tolist() == [29]
    # mixed lengths: 6 edits of 64 letters (slack 6) beat 1 edit of 12 (slack 1)
    assert adapters.name_reads(np.array([[1, 6]], np.uint16), [12, 64], 0.2, 2)[0].tolist() == [1]


def test_patterns_from_the_command_line_and_from_files(tmp_path):
    assert adapters.load_patterns(["acgtacgtacgtac", "TTTTGGGGCCCCAAAA"]) == [("adapter1", "ACGTACGTACGTAC"), ("adapter2", "TTTTGGGGCCCCAAAA")]
    fa = tmp_path / "a.fa"
    fa.write_text(">bc01 first\nACGTACGT\nACGTAC\n>bc02\nttttggggccccaaaa\n")
    assert adapters.load_patterns([str(fa)]) == [("bc01", "ACGTACGTACGTAC"), ("bc02", "TTTTGGGGCCCCAAAA")]
    fq = tmp_path / "a.fq"
    fq.write_text("@bc01 x\nACGTACGTACGTAC\n+\nIIIIIIIIIIIIII\n@bc02\nTTTTGGGGCCCCAAAA\n+\nIIIIIIIIIIIIIIII\n")
    assert adapters.load_patterns([str(fq)]) == adapters.load_patterns([str(fa)])
    good = adapters.load_patterns([str(fa)])
    assert adapters.check(good, 256, 0.2, 2, 20000) is None
    assert "1..64 sequences" in adapters.check([(f"a{i}", "ACGT" * 4) for i in range(65)], 256, 0.2, 2, 20000)
    assert "12..64 letters" in adapters.check([("a", "ACGT" * 2)], 256, 0.2, 2, 20000) and "12..64 letters" in adapters.check([("a", "A" * 65)], 256, 0.2, 2, 20000)
    assert "other letters" in adapters.check([("a", "ACGTN" * 4)], 256, 0.2, 2, 20000)
    for search, maxlen in ((15, 20000), (1025, 20000), (256, 200)):
        assert "--adaptersearch" in adapters.check(good, search, 0.2, 2, maxlen)
    assert "names of their own" in adapters.check([("a", "ACGT" * 4), ("a", "ACGT" * 5)], 256, 0.2, 2, 20000)
