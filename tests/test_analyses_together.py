"""Every read analysis in ONE run of the CLI, on the emulation engines: `--variants`, `--ends --anchor`, `--adapters`, `--refine` and
`--tracts` together leave, file by file and byte for byte, what each of them leaves alone -- on the one-pass route and on the two-pass
route -- and what they left before the analyses went through one dispatch in batch.py and one feature list in main.py
(tests/golden/analyses_together.json).  tests/test_gpu_analyses_together.py runs the two together runs on the GPU."""
import pytest

import together_cases as tg


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{(run, route): output directory} of the eleven runs."""
    root = tmp_path_factory.mktemp("together")
    engines = tg.emu_engines()
    return {(name, route): tg.run(root, engines, name, route, flags) for name, route, flags in tg.RUNS}


@pytest.mark.parametrize("route", ["off", "on"])
def test_together_run_holds_every_single_run_file_by_file(runs, route):
    together = tg.files(runs["together", route])
    seen = set()
    for (name, r), outdir in runs.items():
        if r != route or name == "together":
            continue
        alone = tg.files(outdir)
        assert len(alone) > 2, name                                            # (telolengths_all.csv, the FASTA and the analysis's own)
        for f, b in alone.items():
            assert together[f] == b, (name, route, f)
        seen |= set(alone)
    assert set(together) == seen                                               # ... and has no other files


def test_both_routes_agree_on_every_file_both_have(runs):
    off, on = tg.files(runs["together", "off"]), tg.files(runs["together", "on"])
    assert set(off) - set(on) == {"tracts.csv", "tract_reads.csv"} and not set(on) - set(off)
    for f, b in on.items():
        assert off[f] == b, f
    assert "scanned in two passes" in open(runs["together", "on"] + "/" + tg.LOG).read()


@pytest.mark.parametrize("route", ["off", "on"])
def test_summary_blocks_keep_their_order_in_the_log(runs, route):
    assert tg.summary_order(runs["together", route]) == tg.expected_order(tracts=route == "off")


@pytest.mark.parametrize("route", ["off", "on"])
def test_files_are_those_of_the_golden_hashes(runs, route):
    got, want = tg.hashes(runs["together", route]), tg.golden()[route]
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f
    # the fixture is worth its name: six end groups for either k, and rows in every analysis's file
    lines = {f: b.count(b"\n") for f, b in tg.files(runs["together", route]).items() if f.endswith(".csv")}
    assert lines["ends_4.csv"] == lines["ends_5.csv"] == 7
    for stem in ("variants", "end_reads", "anchored_reads", "adapters", "refined"):
        assert lines[f"{stem}_4.csv"] > 60 and lines[f"{stem}_5.csv"] > 60, stem
    if route == "off":
        assert lines["tracts.csv"] > 60 and lines["tract_reads.csv"] > 60
