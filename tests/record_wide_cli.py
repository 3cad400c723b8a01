"""TEST INFRASTRUCTURE ONLY -- records tests/golden/widecli_*.json: whole runs of the reference's own main() (imported through
oracle/ref_import.py, so only where the reference checkout exists) on motifs of 16 to 32 letters, the tables the wide kernel
scans.  Like tests/golden/reference_runs.json a fixture holds the case's digest (make_case() below rebuilds the seeded input
files), its flags and what the run left behind, the filtered and raw-count files as digests; tests/test_wide_cli.py replays them.  Two k are only ever given with FASTQ input (upstream's FASTA-with-
several-k crash, tests/test_ref_cli_differential.py).

    python tests/record_wide_cli.py            # rewrites every widecli_*.json
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import cli_cases  # noqa: E402

M16, M23, M25, M32 = "CTGTGGGGTCTGGGTG", "ACGGATGTCTAACTTCTTGGTGT", "ACGGATTTGATTAGGTATGTGGTGT", "ACGGATGTCTAACTTCTTGGTGTACGGATTTG"
# name -> (motif, file kind, extra flags, seed)
RUNS = {
    "m16_fastq": (M16, "fastq", ["--cutoff", "0.3"], 1601),
    "m23_fa_gz": (M23, "fa.gz", ["--cutoff", "0.15"], 2301),
    "m25_fasta": (M25, "fasta", ["--cutoff", "0.15", "--slide", "6"], 2501),
    "m32_fastq_gz": (M32, "fastq.gz", ["--cutoff", "0.1"], 3201),
    "m16_rawcount_w150": (M16, "fastq", ["--cutoff", "0.3", "--rawcountpattern", "--windowSize", "150"], 1602),
    "m16_k4_k14": (M16, "fastq", ["--cutoff", "0.3", "--telophrase", "4", "14"], 1603),          # a narrow and a wide table in one run
    "m23_k6_k21": (M23, "fastq", ["--cutoff", "0.15", "--telophrase", "6", "21"], 2302),         # two wide tables
}
MIN_ROWS = 5
MAX_BYTES = 120_000


def make_case(name):
    motif, kind, extra, seed = RUNS[name]
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(12):
        length = int(rng.choice([1500, 1900, 2200, 2600]))
        recs.append((f"w{seed}_{i}", "len=%d" % length if i % 2 else "", cli_cases.make_read(rng, motif, length, telomeric=i % 6 != 5, noisy=i % 3 != 0)))
    fmt = "fastq" if "q" in kind.split(".")[0] else "fasta"
    text = cli_cases.file_text(rng, recs, fmt, wrap=60 if kind == "fasta" else None)
    rel = f"in/reads_{name}.{kind}"
    return {"name": f"widecli_{name}", "files": {rel: text}, "pre": {}, "argv": ["--pattern", motif, "--minSeqLength", "1200", "--threads", "1"] + extra,
            "input": rel, "exit": None}


def record(name):
    """The reference's main() on the case -> the fixture as a JSON string."""
    import ref_import
    case = make_case(name)
    with tempfile.TemporaryDirectory() as d:
        inp, out = cli_cases.materialise(case, d)
        code = ref_import.run_reference_main(["-i", inp, "-o", out] + case["argv"])
        assert code == case["exit"], (name, code)
        expected = cli_cases.digest_outputs(cli_cases.normalise(out))
    rows = len(expected["csv"]) - 1
    assert rows >= MIN_ROWS, (name, rows)
    text = json.dumps({"case_sha256": cli_cases.case_digest(case), "argv": case["argv"], "expected": expected}, sort_keys=True) + "\n"
    assert len(text) <= MAX_BYTES, (name, len(text))
    return text, rows


if __name__ == "__main__":
    for name in RUNS:
        text, rows = record(name)
        with open(os.path.join(GOLD, f"widecli_{name}.json"), "w") as h:
            h.write(text)
        print(f"widecli_{name}.json: {rows} rows, {len(text)} bytes")
