"""TEST INFRASTRUCTURE ONLY -- records tests/golden/wideov_*.json: the rows of the reference's own patterns_vs_match_heatmap
(Topsicle/descriptive_plot.py:233-313, imported through oracle/ref_import.py, so only where the reference checkout exists) on
motifs of 16 to 32 letters and on a short k with more than 8 following letters -- what tps_batch_kmer_followers_wide answers.
Like tests/golden/widecli_*.json a fixture holds the digest of its seeded input (make_case() below rebuilds the FASTQ file),
the call's arguments and what the reference returned: the number of rows, the rows of each strand, the sha256 of all rows in
order, the first 25 rows and, where at most 8 letters follow the k-mer, the crosstab behind the heat map.
tests/test_wide_overview.py replays them through the emulation, tests/test_gpu_wide_overview.py on the GPU.

    python tests/record_wide_overview.py            # rewrites every wideov_*.json
"""
import hashlib
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

M16, M23, M32 = "CTGTGGGGTCTGGGTG", "ACGGATGTCTAACTTCTTGGTGT", "ACGGATGTCTAACTTCTTGGTGTACGGATTTG"
# name -> (motif, k, seed)
RUNS = {
    "m16_k14": (M16, 14, 1611),
    "m23_k21": (M23, 21, 2311),
    "m32_k30": (M32, 30, 3211),          # n_fwd = 32, 64 patterns
    "m23_k6": (M23, 6, 2312),            # 17 following letters: no histogram
    "m32_k4": (M32, 4, 3212),            # 58 patterns, 54 distinct k-mers: groups shared by the two halves of the list
    "m16_k4": (M16, 4, 1612),            # a narrow table with 12 following letters
}
MIN_SEQ_LENGTH = 1200
MIN_ROWS = 1000
MAX_BYTES = 120_000
HIST_MAX_FOLLOW = 8


def make_case(name):
    motif, k, seed = RUNS[name]
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(8):
        length = int(rng.choice([1500, 1900, 2200, 2600]))
        recs.append((f"v{seed}_{i}", "len=%d" % length if i % 2 else "", cli_cases.make_read(rng, motif, length, telomeric=i != 5, noisy=i % 3 != 0)))
    rel = f"in/reads_{name}.fastq"
    return {"name": f"wideov_{name}", "files": {rel: cli_cases.file_text(rng, recs, "fastq")}, "pre": {}, "argv": [motif, str(k), str(MIN_SEQ_LENGTH)],
            "input": rel, "exit": None}


def rows_digest(rows):
    """sha256 of the rows (k-mer, following letters, [read id]) in order."""
    return hashlib.sha256("\n".join(f"{p},{m},{ids[0]}" for p, m, ids in rows).encode()).hexdigest()


def crosstab(rows):
    """The heat map's table of the rows as lists: (patterns = columns, matches = index, counts)."""
    import pandas as pd
    df = pd.DataFrame([(p, m) for p, m, _ids in rows], columns=["Pattern", "Match"])
    tab = pd.crosstab(df["Match"], df["Pattern"])
    return [str(c) for c in tab.columns], [str(i) for i in tab.index], tab.values.astype(int).tolist()


def record(name):
    """The reference's patterns_vs_match_heatmap on the case -> the fixture as a JSON string."""
    import contextlib
    import io
    import matplotlib.pyplot as plt
    import ref_import
    dp = ref_import.load_reference_descriptive_plot()
    motif, k, _seed = RUNS[name]
    case = make_case(name)
    strand_rows = []
    real_concat = dp.pd.concat

    def concat(frames, *a, **kw):               # the reference joins its two strands' rows here: how many each had
        strand_rows.append([int(len(f)) for f in frames])
        return real_concat(frames, *a, **kw)
    with tempfile.TemporaryDirectory() as d:
        inp, _out = cli_cases.materialise(case, d)
        dp.pd.concat = concat
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                df = dp.patterns_vs_match_heatmap(inp, motif, k, MIN_SEQ_LENGTH)
        finally:
            dp.pd.concat = real_concat
            plt.close("all")
    rows = [(str(r[0]), str(r[1]), list(r[2])) for r in df.values.tolist()]
    assert len(strand_rows) == 1 and sum(strand_rows[0]) == len(rows), (name, strand_rows, len(rows))
    assert len(rows) >= MIN_ROWS and min(strand_rows[0]) > 0, (name, len(rows), strand_rows)
    fx = {"case_sha256": cli_cases.case_digest(case), "motif": motif, "k": k, "minSeqLength": MIN_SEQ_LENGTH, "n_rows": len(rows),
          "rows_per_strand": strand_rows[0], "rows_sha256": rows_digest(rows), "first_rows": [[p, m, ids] for p, m, ids in rows[:25]]}
    if len(motif) - k <= HIST_MAX_FOLLOW:
        fx["patterns"], fx["matches"], fx["counts"] = crosstab(rows)
    text = json.dumps(fx, sort_keys=True) + "\n"
    assert len(text) <= MAX_BYTES, (name, len(text))
    return text, len(rows)


if __name__ == "__main__":
    for name in RUNS:
        text, rows = record(name)
        with open(os.path.join(GOLD, f"wideov_{name}.json"), "w") as h:
            h.write(text)
        print(f"wideov_{name}.json: {rows} rows, {len(text)} bytes")
