"""The variant census (tps_batch_variant_census; csrc/tps_variant.h) on the host emulation of its kernel: equal to the plain
restatement of the rule (tests/variant_oracle.py) count for count on every edge the rule and the walk through the tract have
(tests/variant_cases.py), the isolated-variant case whose answer follows from its construction, the library's refusals, the
stand-alone sanitizer run of the same kernel text, and topsicle_amd.variants: names, root reduction, CSV layout."""
import csv
import subprocess

import numpy as np
import pytest

import emu_variant_driver as emu
import variant_cases as vc
import variant_oracle
from topsicle_amd import hiplib, variants


@pytest.mark.parametrize("name", vc.CASE_IDS)
def test_emulation_equals_oracle(name):
    c = vc.case(name)
    shift = vc.CASE_IDS.index(name) & 3
    counts, profile = emu.variant_census(*c.args(), want_profile=True, base_shift=shift, **c.kw())
    vc.assert_equal(counts, profile, name)
    counts, profile = emu.variant_census(*c.args(), want_profile=False, base_shift=shift, **c.kw())
    vc.assert_equal(counts, profile, name, with_profile=False)


def test_cases_reach_what_they_are_for():
    """The edge cases say what they claim to say (on the oracle's answers)."""
    for key, unit in vc.UNITS.items():
        m = len(unit)
        c = vc.case(f"lengths_{key}")
        counts, profile = vc.expected(c.name)
        clamped = np.minimum(np.array(c.end), [len(r) for r in c.reads])
        t = clamped - np.array(c.begin)
        assert (counts[t == m - 1] == 0).all() and (counts[t == m, 0] == 1).all() and (counts[t == m + 1, 0] == 2).all()
        assert {63, 64, 65} <= set(counts[:, 0].tolist())
        assert np.array_equal(counts[:, 0], np.maximum(t - m + 1, 0))
        assert (np.array(c.end) > [len(r) for r in c.reads]).any() and (np.array(c.begin) % 16 != 0).any()
        assert profile[-1, 0] > 0 and profile.sum(axis=0)[0] == counts[:, 0].sum()
        assert (counts[:, [2 + 4 * p + "ACTG".index(unit[p]) for p in range(m)]] == 0).all()          # c = U[p] is always 0
    # the tie of AAAC: AAAA is the variant (p = 3, c = A) whatever rotation it sits in
    counts, _ = variant_oracle.variant_census(["AAACAAAAAAAC"], "AAAC", [0], [0], [12])
    assert counts[0, 0] == 9 and counts[0, 2 + 4 * 3 + 0] == 4 and counts[0, 1] == 5
    counts, _ = vc.expected("ragged")
    assert (counts[np.array(vc.ragged().end) == 0] == 0).all() and counts[:, 0].max() > 8000
    assert vc.expected("empty")[0].shape == (0, 26)
    counts, profile = vc.expected("long_CCCTAA_bin500")
    assert (counts[:, 0] == 20000 - 6 + 1).all() and (profile[:, 0] > 0).all()
    counts, profile = vc.expected("long_CCCTAA_bin64")
    assert profile[-1, 0] == 2 * (20000 - 63 * 64) and profile[0, 0] == 2 * (64 - 5)                 # clipped into the last bin; m - 1 positions short at the boundary


@pytest.mark.parametrize("unit, place, letter, name", vc.ISOLATED)
@pytest.mark.parametrize("tail", [0, 1])
def test_isolated_variants_count_m_each(unit, place, letter, name, tail):
    """Independent of the oracle: each planted unit adds exactly m to its class and takes m from canonical."""
    m, planted = len(unit), 7
    read, begin, end = vc.isolated(unit, place, letter, planted, tail)
    assert variants.class_names(unit)[variants.class_columns(unit).index(2 + 4 * place + "ACTG".index(letter))] == name
    for fn in (emu.variant_census, variant_oracle.variant_census):
        counts, profile = fn([read], unit, [tail], [begin], [end], bin=500, n_bins=40)
        n, canon, other, cls = variants.split_row(counts[0], unit)
        assert n == end - m + 1 and other == 0
        assert dict(zip(variants.class_names(unit), cls))[name] == m * planted and sum(cls) == m * planted
        assert canon == n - m * planted
        assert np.array_equal(profile.sum(axis=0), counts[0].astype(np.int64))


@pytest.mark.parametrize("kw, code", vc.REFUSALS)
def test_refusals_carry_the_librarys_codes(kw, code):
    """TPS_E_ARG (-3) and TPS_E_CAPACITY (-5) as tps_batch_variant_census returns them (test_gpu_variant.py asks the library the same)."""
    a = dict(code=variants.unit_code("CCCTAA")[0], m=6, tails=[0], begin=[0], end=[100], bin=500, n_bins=40)
    a.update(kw)
    with pytest.raises(hiplib.TopsicleHipError) as e:
        emu.variant_census_code(["CCCTAA" * 20], a["code"], a["m"], a["tails"], a["begin"], a["end"], a["bin"], a["n_bins"])
    assert code in str(e.value)


def test_standalone_program_is_clean_under_sanitizers():
    """The same kernel text under -fsanitize=address,undefined, as a program of its own: poisoned LDS of exactly one wave's size,
    garbage around the batch, a ragged batch checked against its own restatement of the rule."""
    exe = emu.build_main()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


def test_unit_code_root_and_names():
    assert variants.unit_code("CCCTAA") == (sum(v << (2 * j) for j, v in enumerate([1, 1, 1, 2, 0, 0])), 6)
    assert variants.code_unit(*variants.unit_code(vc.M32)) == vc.M32 and variants.unit_code(vc.M32)[0] >> 62 != 0
    assert variants.primitive_root("CCCTAACCCTAA") == "CCCTAA" and variants.primitive_root("AAAA") == "A"
    assert variants.primitive_root("CCCTAA") == "CCCTAA" and variants.primitive_root("CCACCA") == "CCA"
    with pytest.raises(ValueError):
        variants.unit_code("CCNTAA")
    with pytest.raises(ValueError):
        variants.unit_code("A" * 33)
    names = variants.class_names("CCCTAA")
    assert len(names) == 18 and names[:3] == ["C1A", "C1G", "C1T"] and names[9:12] == ["T4A", "T4C", "T4G"] and names[-1] == "A6T"
    cols = variants.class_columns("CCCTAA")
    assert cols[:3] == [2 + 0, 2 + 3, 2 + 2] and cols[10] == 2 + 4 * 3 + 1 and len(set(cols)) == 18
    assert variants.VariantSpec("ccctaaccctaa").unit == "CCCTAA"


def test_csv_layout_and_summary(tmp_path):
    unit = "CCCTAA"
    row = np.zeros(26, np.uint32)
    row[0], row[1], row[2 + 4 * 3 + 1], row[2 + 4 * 5 + 3] = 100, 70, 12, 6
    p = tmp_path / "variants_4.csv"
    variants.write_reads_csv(p, unit, [("f.fq", "read1", 1, 100, 205, row)])
    got = list(csv.reader(open(p)))
    assert got[0] == ["file", "readID", "tail", "tract_begin", "tract_end", "positions", "canonical", "other"] + variants.class_names(unit)
    assert got[1][:8] == ["f.fq", "read1", "reverse", "100", "205", "100", "70", "12"]
    assert dict(zip(got[0], got[1]))["T4C"] == "12" and dict(zip(got[0], got[1]))["A6G"] == "6" and len(got) == 2
    prof = np.zeros((3, 26), np.int64)
    prof[1] = row
    q = tmp_path / "variant_profile_4.csv"
    variants.write_profile_csv(q, unit, prof, 500)
    got = list(csv.reader(open(q)))
    assert got[0] == ["bin_start", "positions", "canonical", "other"] + variants.class_names(unit) and len(got) == 4
    assert [r[0] for r in got[1:]] == ["0", "500", "1000"] and got[2][1:4] == ["100", "70", "12"] and got[1][1:4] == ["0", "0", "0"]
    lines = variants.summary(unit, row, 1)
    assert len(lines) == 5 and "70.00%" in lines[1] and "T4C 12.00% (~2 units)" in lines[3] and "A6G" in lines[3]
    assert len(variants.summary(unit, np.zeros(26, np.uint32), 0)) == 5
