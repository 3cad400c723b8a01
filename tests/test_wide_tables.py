"""The wide-table scan kernel (csrc/tps_wide.h: k <= 32 letters, P <= 64 patterns) compiled as a sequential host emulation
(tests/emu/emu_wide.cpp) against oracle/oracle.c, bit for bit, on the seeded case matrix of tests/wide_cases.py.  The same
matrix runs through the real kernel in tests/test_gpu_wide.py."""
import numpy as np
import pytest

import emu_driver
import emu_wide_driver as emuw
import wide_cases
from emu_wide_engine import EmuWideEngine
from topsicle_amd import hiplib

CASES = wide_cases.cases()


def test_case_matrix_covers_what_it_promises():
    assert len(CASES) >= 300
    ks = {len(c["patterns"][0]) for c in CASES}
    ps = {len(c["patterns"]) for c in CASES}
    assert {6, 14, 16, 21, 23, 24, 30, 32} <= ks and max(ks) == 32
    assert {32, 46, 50, 52, 64} <= ps and max(ps) == 64
    assert {c["mode"] for c in CASES} == {"sums", "raw", "tails", "step1"}
    assert {c["W"] for c in CASES} == {100, 60, 150, 300} and {c["s"] for c in CASES} >= {6, 7, 1, 25, 16, 23, 32}
    assert any(len(s) == 0 for c in CASES for s in c["seqs"]) and any(len(s) == 60000 for c in CASES for s in c["seqs"])
    assert any("N" in s for c in CASES for s in c["seqs"]) and any(s and s == s.lower() for c in CASES for s in c["seqs"])


def test_hash_tables_hold_every_distinct_kmer_once():
    for name, pats in list(wide_cases.made_up_tables().items()) + [(n, p) for n, _, p in wide_cases.motif_tables()]:
        t = emuw.table(pats)
        assert t["n_groups"] == t["used"] == len(set(pats)), name
        so = {p for p in pats if any(p[d:] == p[:-d] for d in range(1, len(p)))}
        assert t["n_so"] == len(so), name
    assert emuw.table(["G" * 32])["mask_hi"] == 0xFFFFFFFF       # the all-G 32-mer: a code of all ones, a legal key


@pytest.mark.parametrize("chunk", range(10))
def test_wide_kernel_emulation_matches_the_c_oracle(chunk):
    rng = np.random.default_rng(chunk)
    windows = 0
    for ci, c in enumerate(CASES):
        if ci % 10 != chunk:
            continue
        tails = wide_cases.tails_for(c, rng) if c["mode"] == "tails" else None
        out = emuw.scan(c["patterns"], c["seqs"], wide_cases.params_of(c), tails=tails, base_shift=ci % 4)
        windows += wide_cases.check_output(c, out, tails)
    assert windows > 0


def test_narrow_table_through_both_emulations_is_the_same_scan():
    c = next(c for c in CASES if c["name"].endswith("narrow_ccctaa_k4") and c["mode"] == "raw")
    prm = wide_cases.params_of(c)
    emu_driver.build()
    narrow = emu_driver.scan(c["patterns"], c["seqs"], prm)
    wide = emuw.scan(c["patterns"], c["seqs"], prm)
    for key in ("c_start", "c_end", "win_off", "sums", "raw"):
        assert np.array_equal(narrow[key], wide[key]), key
    for f in ("best_start", "best_start_idx", "best_end", "best_end_idx", "tail", "pass", "n_win"):
        assert np.array_equal(narrow["results"][f], wide["results"][f]), f


def test_limits_are_loud():
    eng = EmuWideEngine()
    for bad in (["A" * 33], ["ACGT" * 4 + "ACG" + "ACGT"[i % 4] + "ACGT"[i // 4 % 4] + "ACGT"[i // 16 % 4] for i in range(64)] + ["T" * 22], ["ACGN"], []):
        with pytest.raises(hiplib.TopsicleHipError):
            eng.set_patterns_wide(bad)
    eng.set_patterns_wide(["ACGT" * 5])
    eng.upload(0, *hiplib.pack_reads(["ACGT" * 500]))
    with pytest.raises(hiplib.TopsicleHipError):
        eng.kmer_followers(0, 1, 2)
    with pytest.raises(hiplib.TopsicleHipError):       # a window that can hold more than 255 occurrences of a k-mer
        emuw.scan(["A"], ["ACGT" * 500], hiplib.make_params(window=300, flags=hiplib.F_WINDOWS))
    assert hiplib.needs_wide(["A" * 16]) and hiplib.needs_wide(["ACGT"] * 32) and not hiplib.needs_wide(["A" * 15] * 31)
    assert (hiplib.WIDE_MAX_K, hiplib.WIDE_MAX_PATTERNS, hiplib.MAX_K, hiplib.MAX_PATTERNS) == (32, 64, 15, 31)
