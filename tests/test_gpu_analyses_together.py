"""Every read analysis in one run of the CLI on the GPU: the two together runs of tests/test_analyses_together.py (one pass with the
tract map, two passes without) on two contexts of device 0 -- the routes agree file by file, and the files are those of the golden
hashes, which the emulation engines give too.  No kernel and no launch shape of its own: tests/test_gpu_*.py hold each analysis
against its emulation bit for bit."""
import pytest

import together_cases as tg
from topsicle_amd import hiplib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("together_gpu")
    engines = [hiplib.HipScanner(0), hiplib.HipScanner(0)]
    try:
        return {route: tg.run(root, engines, "together", route, flags) for name, route, flags in tg.RUNS if name == "together"}
    finally:
        for e in engines:
            e.close()


def test_both_routes_agree_on_every_file_both_have(runs):
    off, on = tg.files(runs["off"]), tg.files(runs["on"])
    assert set(off) - set(on) == {"tracts.csv", "tract_reads.csv"} and not set(on) - set(off)
    for f, b in on.items():
        assert off[f] == b, f
    assert "scanned in two passes" in open(runs["on"] + "/" + tg.LOG).read()


@pytest.mark.parametrize("route", ["off", "on"])
def test_files_are_those_of_the_golden_hashes(runs, route):
    got, want = tg.hashes(runs[route]), tg.golden()[route]
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f
    assert tg.summary_order(runs[route]) == tg.expected_order(tracts=route == "off")
