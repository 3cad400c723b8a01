"""The k-mer / follower counts of the overview heat map on WIDE tables (followers_wide_read in csrc/tps_wide.h,
tps_batch_kmer_followers_wide): motifs of 16 to 32 letters, and any k that leaves more than 8 letters to follow.  The kernel
source runs here as the sequential host emulation (tests/emu/emu_follow_wide.cpp); tests/test_gpu_wide_overview.py runs the
same checks (tests/wide_overview_checks.py) through the C ABI.

  * the rows the reference's own patterns_vs_match_heatmap returned (tests/golden/wideov_*.json, tests/record_wide_overview.py);
  * random reads against oracle.kmer_followers: lengths around every limit, N / IUPAC / lower-case letters, both orientations;
  * picks and histogram bit-identical to the narrow kernel's on tables both take;
  * the refusals; one run under AddressSanitizer / UBSan; overview_plot end to end.
"""
import os
import sys

import pytest

import record_wide_overview as rec
import wide_overview_checks as chk
from topsicle_amd import allsteps


@pytest.fixture()
def engine():
    from emu_follow_wide_engine import EmuFollowWideEngine
    e = EmuFollowWideEngine()
    allsteps.set_engine(e)
    yield e
    allsteps.set_engine(None)


def test_fixtures_are_what_the_issue_asks_for(gold_dir):
    import json
    assert sorted(rec.RUNS) == sorted(f[len("wideov_"):-len(".json")] for f in os.listdir(gold_dir) if f.startswith("wideov_"))
    shapes = set()
    for name in rec.RUNS:
        path = os.path.join(gold_dir, f"wideov_{name}.json")
        fx = json.load(open(path))
        assert os.path.getsize(path) <= rec.MAX_BYTES
        assert fx["n_rows"] >= 1000 and min(fx["rows_per_strand"]) > 0 and sum(fx["rows_per_strand"]) == fx["n_rows"]
        assert ("counts" in fx) == (len(fx["motif"]) - fx["k"] <= 8)
        shapes.add((len(fx["motif"]), fx["k"]))
    assert shapes == {(16, 14), (23, 21), (32, 30), (23, 6), (32, 4), (16, 4)}
    # the 32-letter motif at k = 4: fewer distinct k-mers than patterns, groups shared by the two halves of the list
    table = allsteps.patterns_to_search(rec.M32, 4)
    assert len(table) == 58 and len(set(table)) == 54
    assert len(allsteps.patterns_to_search(rec.M32, 30)) == 64


@pytest.mark.parametrize("name", list(rec.RUNS))
def test_rows_equal_reference_emulation(name, gold_dir, tmp_path, engine):
    chk.check_fixture(name, gold_dir, tmp_path, engine)


@pytest.mark.parametrize("seed", range(14))
def test_followers_wide_random_vs_oracle_emulation(engine, seed):
    chk.check_random_reads_against_oracle(engine, seed)


def test_wide_entry_equals_narrow_entry_emulation(engine):
    chk.check_old_against_new(engine)


def test_error_paths_are_loud_emulation(engine):
    chk.check_error_paths(engine)


def test_batch_moved_inside_its_buffer_emulation():
    """The packed batch at every quad offset inside its buffer, garbage around it: the same picks."""
    import numpy as np
    import emu_follow_wide_driver as emuf
    table = allsteps.patterns_to_search(rec.M23, 6)
    seqs = chk.random_reads(np.random.default_rng(5), rec.M23, [1999, 2001, 64, 5000, 130])
    base = emuf.followers_wide(table, seqs, 23, 17, want_hist=False)[0]
    assert base.any()
    for shift in (1, 2, 3):
        assert np.array_equal(emuf.followers_wide(table, seqs, 23, 17, want_hist=False, base_shift=shift)[0], base)


def test_followers_wide_emulation_under_asan_ubsan():
    """The kernel source with every LDS / global index checked: random reads of every shape, old against new, the moved batch."""
    import test_sanitizers as ts
    sys.path.insert(0, os.path.join(ts.ROOT, "tests"))
    import emu_driver
    import emu_follow_wide_driver
    import emu_wide_driver
    emu_driver.build(asan=True)
    emu_wide_driver.build(asan=True)
    emu_follow_wide_driver.build(asan=True)
    out = ts._run_under_sanitizers(["tests/test_wide_overview.py", "-k", "random_vs_oracle or equals_narrow or moved_inside or error_paths"],
                                   {"TPS_EMU_ASAN": "1"})
    assert " passed" in out and "skipped" not in out.split("passed")[-1]


@pytest.mark.parametrize("motif", list(chk.E2E_MOTIFS))
def test_overview_driver_long_motif_with_emulation(tmp_path, engine, motif):
    chk.check_overview_end_to_end(tmp_path, chk.E2E_MOTIFS[motif], [engine])


def test_heat_map_numbers_only_where_they_fit(gold_dir, tmp_path, engine):
    """Up to 8 following letters every cell carries its count, as before; beyond that only a grid of at most MAX_CELLS_ANNOTATED cells."""
    import matplotlib.pyplot as plt
    from topsicle_amd import descriptive_plot as dp
    for name, annotated in (("m23_k21", True), ("m23_k6", False)):
        fx, recs = chk.fixture_records(name, gold_dir, tmp_path / name)
        table = dp.heatmap_from_records(recs, name, fx["motif"], fx["k"], fx["minSeqLength"], engine)
        cells = table["Match"].nunique() * table["Pattern"].nunique()
        texts = len(plt.gcf().axes[0].texts)
        plt.close("all")
        assert len(table) == fx["n_rows"]
        assert (cells > dp.MAX_CELLS_ANNOTATED) == (not annotated) and texts == (cells if annotated else 0), (name, cells, texts)
