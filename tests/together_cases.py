"""Every read analysis of the CLI in one run (tests/test_analyses_together.py on the emulation engines,
tests/test_gpu_analyses_together.py on the GPU): the inputs, the eleven runs, the files they leave and the golden hashes of the two
runs with everything switched on (tests/golden/analyses_together.json: every CSV and the FASTA; the PNGs depend on the matplotlib
build).  `PYTHONPATH=.:oracle python tests/together_cases.py DIR` leaves the eleven runs on the emulation engines under DIR."""
import hashlib
import json
import os
import re

import ends_cases as ec
from topsicle_amd import main as cli

IDENT = "CCCTAA_ONT"
ADAPTERS = ["GATTACAGGCATCGTTC", "TGCATCAGGTCCAAGTCA", "CAGTTGACCATGGATCCTA", "AGGTCTTCAGCAGTTGACCA"]          # 17, 18, 19, 20 letters
COMMON = ["--pattern", "CCCTAACCCTAA", "--telophrase", "4", "5", "--minSeqLength", "5000", "--cutoff", "0.4"]
FEATURES = {"variants": ["--variants"], "anchor": ["--ends", "--anchor"], "adapters": ["--adapters"] + ADAPTERS, "refine": ["--refine"],
            "tracts": ["--tracts"]}
ALL = sum(FEATURES.values(), [])
ALL_BUT_TRACTS = sum((f for name, f in FEATURES.items() if name != "tracts"), [])
# (run, route, flags): each analysis alone on both routes -- the tract map needs whole reads --, then all of them together
RUNS = [(name, route, flags) for name, flags in FEATURES.items() for route in ("off", "on") if (name, route) != ("tracts", "on")] + \
       [("together", "off", ALL), ("together", "on", ALL_BUT_TRACTS)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analyses_together.json")
LOG = "topsicle_run.log"
# the first summary line of every analysis, in the order the log has them
FIRST_LINES = {"variants": "variant census of ", "ends": "end groups against ", "anchor": "anchored lengths: ", "adapters": "adapters: 4 sequences",
               "refine": "refined boundaries: ", "tracts": "tract map of "}


def build_emulations():
    import emu_adapter_driver
    import emu_anchor_driver
    import emu_driver
    import emu_ends_driver
    import emu_follow_wide_driver
    import emu_motif_driver
    import emu_refine_driver
    import emu_tract_driver
    import emu_variant_driver
    import emu_wide_driver
    for d in (emu_driver, emu_wide_driver, emu_follow_wide_driver, emu_motif_driver, emu_variant_driver, emu_tract_driver, emu_ends_driver,
              emu_anchor_driver, emu_adapter_driver, emu_refine_driver):
        d.build()


def every_engine():
    """The class of a context that has every read-analysis call: EmuRefineEngine with EmuTractEngine's tract_map mixed in."""
    build_emulations()
    from emu_refine_engine import EmuRefineEngine
    from emu_tract_engine import EmuTractEngine

    class EmuEveryEngine(EmuRefineEngine):
        tract_map = EmuTractEngine.tract_map

        def helper(self, j):
            hs = self.__dict__.setdefault("_helpers", [])
            while len(hs) <= j:
                hs.append(type(self)())
            return hs[j]
    return EmuEveryEngine


def emu_engines():
    cls = every_engine()
    return [cls(), cls()]


def run(root, engines, name, route, flags):
    """One run into root/<name>_<route>; the input file is written on first use."""
    d = os.path.join(str(root), "in")
    if not os.path.isdir(d):
        os.makedirs(d)
        ec.write_fasta(os.path.join(d, "reads.fasta"), ec.detection_reads(IDENT)[0])
    out = os.path.join(str(root), f"{name}_{route}")
    args = cli.build_parser().parse_args(["-i", d, "-o", out] + COMMON + flags + ["--twopass", route])
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)
    return out


def files(outdir):
    """{name: bytes} of every file of a run but its log."""
    return {f: open(os.path.join(outdir, f), "rb").read() for f in sorted(os.listdir(outdir)) if f != LOG}


def hashes(outdir):
    """{name: sha256} of a run's CSVs and its FASTA."""
    return {f: hashlib.sha256(b).hexdigest() for f, b in files(outdir).items() if f.endswith((".csv", ".fasta"))}


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def summary_order(outdir):
    """The analyses whose first summary line the log has, in the log's order."""
    got = []
    for line in open(os.path.join(outdir, LOG)):
        msg = re.sub(r"^\[[^\]]*\] ", "", line)
        got += [name for name, start in FIRST_LINES.items() if msg.startswith(start)]
    return got


def expected_order(tracts):
    """Per k: variants; ends with the anchored lengths inside; adapters; refine -- then the one tract map."""
    return ["variants"] * 2 + ["ends", "anchor"] * 2 + ["adapters"] * 2 + ["refine"] * 2 + (["tracts"] if tracts else [])


if __name__ == "__main__":
    import sys
    engines = emu_engines()
    for name, route, flags in RUNS:
        run(sys.argv[1], engines, name, route, flags)
    if len(sys.argv) > 2:                          # (how tests/golden/analyses_together.json was made)
        with open(sys.argv[2], "w") as fh:
            json.dump({route: hashes(os.path.join(sys.argv[1], f"together_{route}")) for route in ("off", "on")}, fh, indent=1, sort_keys=True)
            fh.write("\n")
