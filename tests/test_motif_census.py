"""The motif census (tps_batch_motif_census; csrc/tps_motif.h) on the host emulation of its kernel: equal to the plain restatement
of the rule (tests/motif_oracle.py) field for field and count for count on every edge the rule has (tests/motif_cases.py), the
library's refusals, the stand-alone sanitizer run of the same kernel text, and the vote (topsicle_amd.motif.tally) on the synthetic
read sets the support floor was chosen on."""
import subprocess

import numpy as np
import pytest

import emu_motif_driver as emu
import motif_cases as mc
import motif_oracle
from topsicle_amd import hiplib, motif, synth


@pytest.mark.parametrize("name", mc.CASE_IDS)
def test_emulation_equals_oracle(name):
    _, reads, kw = next(c for c in mc.cases() if c[0] == name)
    shift = mc.CASE_IDS.index(name) & 3
    hits, counts = emu.motif_census(list(reads), want_counts=True, base_shift=shift, **kw)
    mc.assert_equal(hits, counts, name)
    hits, counts = emu.motif_census(list(reads), want_counts=False, base_shift=shift, **kw)
    mc.assert_equal(hits, counts, name, with_counts=False)


def test_cases_reach_what_they_are_for():
    """The edge cases say what they claim to say (on the oracle's answers)."""
    reads = mc.pool()
    homo, perfect, m32 = reads.index("A" * 5000), reads.index("CCCTAA" * 1000), reads.index(mc.M32 * 150)
    h, c = mc.expected("span4096")
    # a homopolymer: every period has every position it can have, the smallest wins, ONE run across all 128 words
    assert [int(x) for x in c[homo, 0]] == [4096 - u - min(u, 8) + 1 for u in range(4, 33)]
    assert tuple(h[homo, 0][["period", "support", "run_start", "run_len", "n_bases"]]) == (4, 4089, 0, 4089, 4096)
    assert tuple(h[homo, 1][["period", "unit"]]) == (4, 0b10101010)                   # the reverse complement reads TTTT
    assert tuple(h[perfect, 0][["period", "run_len"]]) == (6, 4096 - 12 + 1)
    h, _ = mc.expected("u32_only")
    assert h[m32, 0]["period"] == 32 and motif.unit_string(h[m32, 0]["unit"], 32) == mc.M32 and h[m32, 0]["unit"] >> 62 != 0
    for u in (1, 6, 12, 32):
        h0, _ = mc.expected(f"n_eq_u{u}_w_minus1")
        h1, _ = mc.expected(f"n_eq_u{u}_w")
        assert not h0["support"].any() and h1["support"].max() == 1
    h, _ = mc.expected("span1")
    assert not h["support"].any()
    h, _ = mc.expected("min_len")
    short = [i for i, r in enumerate(reads) if len(r) <= 820]
    assert len(reads[short[-1]]) <= 820 and not h[short]["n_bases"].any() and h["n_bases"].any()
    assert any(len(r) == 820 for r in reads)
    h, _ = mc.expected("u1_to_32")
    assert h[homo, 0]["period"] == 1
    assert mc.expected("empty")[0].shape == (0, 2)
    # an N inside the unit (behind its first 8 letters) keeps the packed batch's code
    h, _ = mc.expected("u32_only")
    withn = reads.index(mc.M32[:20] + "N" + mc.M32[21:] + mc.M32[:19])
    assert h[withn, 0]["period"] == 32 and h[withn, 0]["run_start"] == 0 and motif.unit_string(h[withn, 0]["unit"], 32)[20] == "G"


@pytest.mark.parametrize("kw, code", mc.REFUSALS)
def test_refusals_carry_the_librarys_codes(kw, code):
    """TPS_E_ARG (-3) for the periods, TPS_E_CAPACITY (-5) for the range, as tps_batch_motif_census returns them (test_gpu_motif.py
    asks the library the same)."""
    with pytest.raises(hiplib.TopsicleHipError) as e:
        emu.motif_census(["ACGT" * 100], **kw)
    assert code in str(e.value)


def test_standalone_program_is_clean_under_sanitizers():
    """The same kernel text under -fsanitize=address,undefined, as a program of its own: poisoned LDS of exactly one wave's size,
    garbage around the batch, every answer checked against its own restatement of the rule."""
    exe = emu.build_main()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


def test_unit_string_and_canonical():
    assert motif.unit_string(sum(v << (2 * j) for j, v in enumerate([1, 1, 1, 2, 0, 0])), 6) == "CCCTAA"
    assert motif.canonical("CCCTAA") == "AACCCT" and motif.canonical("TAACCC") == "AACCCT"
    assert motif.canonical("CCCTAAA") == "AAACCCT"
    assert motif.canonical("CCCTAACCCTAA") == "AACCCT" and motif.canonical("AAAA") == "A"
    assert motif.canonical("TTAGGG") == "AGGGTT" != motif.canonical("CCCTAA")            # no reverse complement
    assert motif.canonical(mc.M32) == min(mc.M32[i:] + mc.M32[:i] for i in range(32))


def test_tally_ranks_and_floors():
    code = lambda s: sum("ACTG".index(c) << (2 * j) for j, c in enumerate(s))      # noqa: E731
    hits = np.zeros((4, 2), hiplib.MOTIF_HIT_DTYPE)
    for (r, e), (unit, support) in {(0, 0): ("CCCTAA", 100), (1, 1): ("TAACCC", 50), (2, 0): ("TTAGGG", 500), (2, 1): ("CCCTAACCCTAA", 24),
                                    (3, 0): ("ACGTT", 23)}.items():
        hits[r, e] = (code(unit), len(unit), support, 0, support, 1000, 0)
    assert motif.tally(hits) == [("AACCCT", 6, 3, 174), ("AGGGTT", 6, 1, 500)]
    assert motif.tally(hits, min_support=23)[-1] == ("ACGTT", 5, 1, 23)
    assert motif.tally(hits[:0]) == [] and motif.tally(np.zeros((3, 2), hiplib.MOTIF_HIT_DTYPE), min_support=0) == []
    assert motif.verdict([]) and motif.verdict([("AACCCT", 6, 4, 400)]) and motif.verdict([("AACCCT", 6, 5, 400)]) is None


@pytest.mark.parametrize("errors", [synth.ONT, synth.HIFI], ids=["ont", "hifi"])
@pytest.mark.parametrize("name", list(mc.MOTIFS))
def test_vote_finds_the_motif(name, errors):
    """200 reads of 6000 bases, half of them telomeric (tracts of 300 .. 3000 bases), the census with its defaults: the rank-1 motif
    is canonical(motif) and holds at least 90 % of the votes -- first on the oracle's hits alone, then on the emulation's."""
    reads = mc.vote_reads(name, errors)
    want = motif.canonical(mc.MOTIFS[name])
    o_hits, _ = motif_oracle.motif_census(reads)
    e_hits, _ = emu.motif_census(reads)
    for hits in (o_hits, e_hits):
        rows = motif.tally(hits)
        assert rows and rows[0][0] == want, rows[:3]
        assert rows[0][2] >= 0.9 * sum(r[2] for r in rows), rows[:5]
        assert rows[0][2] >= motif.MIN_READ_ENDS
    assert all(np.array_equal(o_hits[f], e_hits[f]) for f in hiplib.MOTIF_HIT_DTYPE.names)
