"""CLI-level differential against the REFERENCE'S OWN main(): Topsicle/main.py is imported unchanged in the
build container (oracle/ref_import.py: Bio / seaborn / ruptures stand-ins, a functional SeqIO.write) and run on seeded random
inputs and flag sets (oracle/cli_cases.py: 1 - 3 files, fasta / fastq / gz, reads around --minSeqLength and --maxlengthtelo,
--telophrase / --cutoff lists, --slide, --trimfirst, --windowSize, --read_check, --override, a pre-existing telolengths_all.csv);
topsicle_amd.main runs the same command on the emulated engines.  Compared: the CSV as a row SEQUENCE, the summary lines of the
log, the filtered files by name and content, the exit code.  The reference's side of every run was recorded by oracle/gen_golden.py
(tests/golden/reference_runs.json: outputs as digests; tests/golden/cli_*.json: whole runs with their inputs, also replayed on the
GPU), so the tests need nothing outside the repository."""
import json
import os

import pytest

import cli_cases
from topsicle_amd import main as cli


@pytest.fixture(scope="module")
def recorded(gold_dir):
    """The reference's runs (oracle/gen_golden.py gen_reference_runs)."""
    return json.load(open(os.path.join(gold_dir, "reference_runs.json")))


def recorded_run(rec, case):
    assert rec["case_sha256"] == cli_cases.case_digest(case), "the case generator changed: re-record with oracle/gen_golden.py"
    return rec


def compare_recorded(rec, inp, b, what):
    """A recorded run of the reference against the product's run on the same case.  When the product visited the input files in
    the recorded order (always for one file), everything is compared exactly: the CSV as a row SEQUENCE, the summary lines, every
    filtered and raw-count file by digest.  Only when this file system walks the input directory in another order does the
    comparison fall back to compare_replayed (rows per file and k; raw-count contents of one-file runs)."""
    a = rec["expected"]
    if cli_cases.walk_order(inp) != rec["walk"]:
        compare_replayed(a, b, what)
        return
    assert a["csv"] == b["csv"], (what, "csv rows")
    assert a["summary"] == b["summary"], (what, "summary lines")
    for kind in ("filtered", "rawcount"):
        assert sorted(a[kind]) == sorted(b[kind]), (what, kind, "file names")
        for f, d in a[kind].items():
            assert d == cli_cases.digest(b[kind][f]), (what, f)


def run_product(engines, argv):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    try:
        cli.analysis_run(args, engines=engines)
    except SystemExit as e:
        return e.code if e.code is not None else 0
    return None


@pytest.mark.parametrize("first", cli_cases.DIFFERENTIAL_FIRST_SEEDS)
def test_cli_matches_the_reference_main(first, tmp_path, emu_engine_factory, recorded):
    """Twelve seeded cases per call.  The reference itself crashes on some inputs the generator can produce -- FASTA input with
    several k: the second k REUSES the first k's `.fasta` (main.py:64-66) and a read that passes only at the second k is not in it,
    so `bound_res[0]` raises IndexError (main.py:131) -- those cases are counted, not compared (the product completes them)."""
    crashed = []
    for seed in range(first, first + 12):
        case = cli_cases.make_case(seed)
        rec = recorded_run(recorded["seeds"][str(seed)], case)
        if "crashed" in rec:
            crashed.append((seed, rec["crashed"]))
            continue
        inp_p, out_p = cli_cases.materialise(case, str(tmp_path / f"prod{seed}"))
        code_p = run_product(emu_engine_factory(), ["-i", inp_p, "-o", out_p] + case["argv"])
        assert rec["exit"] == code_p == case["exit"], (seed, case["argv"], rec["exit"], code_p)
        compare_recorded(rec, inp_p, cli_cases.normalise(out_p), (seed, case["argv"]))
    assert len(crashed) <= 3, crashed


@pytest.fixture(scope="module")
def recorded_long(gold_dir):
    """The reference's runs on the long cases (oracle/gen_golden.py gen_reference_long_runs)."""
    return json.load(open(os.path.join(gold_dir, "reference_long_runs.json")))


def replay_long_case(seed, recorded_long, root, run):
    """One recorded long case (cli_cases.make_long_case: reads of 25 000 to 48 000 bases, --maxlengthtelo 30 000 / 45 000), regenerated
    from its seed and run with `run(argv)` -> exit code; returns the recorded CSV rows."""
    case = cli_cases.make_long_case(seed)
    rec = recorded_run(recorded_long["seeds"][str(seed)], case)
    inp, out = cli_cases.materialise(case, root)
    code = run(["-i", inp, "-o", out] + case["argv"])
    assert rec["exit"] == code == case["exit"], (seed, case["argv"], rec["exit"], code)
    compare_recorded(rec, inp, cli_cases.normalise(out), (seed, case["argv"]))
    return rec["expected"]["csv"][1:]


def test_cli_matches_the_reference_main_beyond_the_default_maxlengthtelo(tmp_path, emu_engine_factory, recorded_long):
    """The four long cases: --maxlengthtelo 30 000 and 45 000 with --slide 6 and 10, one with --rawcountpattern.  The recording holds
    boundaries beyond 20 000 -- what no other recorded run has."""
    rows = []
    for seed in cli_cases.LONG_SEEDS:
        rows += replay_long_case(seed, recorded_long, str(tmp_path / f"long{seed}"), lambda argv: run_product(emu_engine_factory(), argv))
    argvs = [cli_cases.make_long_case(s)["argv"] for s in cli_cases.LONG_SEEDS]
    pick = lambda flag: {a[a.index(flag) + 1] for a in argvs}
    assert pick("--maxlengthtelo") == {"30000", "45000"} and pick("--slide") == {"6", "10"}
    assert sum("--rawcountpattern" in a for a in argvs) == 1
    assert len(rows) >= 20 and sum(1 for r in rows if int(r[4]) > 20000) >= 8


def test_existing_fasta_temp_file_is_reused_like_upstream(tmp_path, emu_engine_factory, recorded):
    """main.py:64-66: a `<name>_trc_over_<cutoff>.fasta` that is already there is used, not rewritten -- also for FASTQ input."""
    # the file the first run wrote = every record as FASTA (upstream's step 2 reads ITS records; the product scans the input)
    case, fasta = cli_cases.existing_fasta_case()
    rec = recorded_run(recorded["existing_fasta"], case)
    inp_p, out_p = cli_cases.materialise(case, str(tmp_path / "prod"))
    assert rec["exit"] is None
    assert run_product(emu_engine_factory(), ["-i", inp_p, "-o", out_p] + case["argv"]) is None
    compare_recorded(rec, inp_p, cli_cases.normalise(out_p), "existing fasta")
    assert rec["expected"]["filtered"][fasta] == cli_cases.digest(case["pre"][fasta])
    assert "Using existing file" in open(os.path.join(out_p, "topsicle_run.log")).read()


def compare_replayed(a, b, what):
    """A recorded run against a replay on ANOTHER machine: both CLIs list a directory with os.walk, whose order is the file system's
    (the fixtures were recorded in the build container; the GPU box's scratch directory orders the same three names differently).
    So: per (k, file) the row SEQUENCE must be equal, the k's must come in the recorded order, and the files in ONE order for every k
    -- everything else (summary lines, filtered files) is compared as it is.  Filtered files recorded as digests are compared by digest."""
    def blocks(rows):
        out, order = {}, []
        for r in rows[1:]:
            key = (r[1], r[0])
            if key not in out:
                out[key] = []
                order.append(key)
            else:
                assert order[-1] == key, (what, "rows of one file and k are not contiguous", key)
            out[key].append(r)
        return out, order
    assert (a["csv"] is None) == (b["csv"] is None)
    if a["csv"] is not None:
        assert a["csv"][0] == b["csv"][0]
        ba, oa = blocks(a["csv"])
        bb, ob = blocks(b["csv"])
        assert ba == bb, (what, "csv rows per file and k")
        ks = lambda order: [k for i, (k, _f) in enumerate(order) if i == 0 or order[i - 1][0] != k]
        assert ks(oa) == ks(ob), (what, "order of the k-mer lengths")
        per_k = {}
        for k, f in ob:
            per_k.setdefault(k, []).append(f)
        full = max(per_k.values(), key=len) if per_k else []
        for k, fs in per_k.items():
            assert fs == [f for f in full if f in fs], (what, "file order differs between k-mer lengths", per_k)
    assert a["summary"] == b["summary"], (what, "summary lines")
    assert sorted(a["filtered"]) == sorted(b["filtered"]), (what, "filtered file names")
    for f in a["filtered"]:
        want = a["filtered"][f]
        assert want == (cli_cases.digest(b["filtered"][f]) if isinstance(want, dict) else b["filtered"][f]), (what, f)
    # rawcount_{k}_{i}.csv is numbered per input file (main.py:90, 150): runs over several files leave, under each name, the LAST file's
    # read -- walk order again -- so their contents are compared for one-file runs only (recorded as digests)
    assert sorted(a.get("rawcount", {})) == sorted(b.get("rawcount", {})), (what, "raw-count file names")
    if len({r[0] for r in (a["csv"] or [])[1:]}) <= 1:
        for f, d in a.get("rawcount", {}).items():
            assert d == cli_cases.digest(b["rawcount"][f]), (what, f)


def golden_cases(gold_dir):
    return sorted(f for f in os.listdir(gold_dir) if f.startswith("cli_") and f.endswith(".json"))


def test_cli_golden_cases(gold_dir, tmp_path, emu_engine_factory):
    """The runs oracle/gen_golden.py recorded from the reference's main(): replayed on the emulated engines."""
    names = golden_cases(gold_dir)
    assert len(names) >= 5
    for n in names:
        g = json.load(open(os.path.join(gold_dir, n)))
        inp, out = cli_cases.materialise(g["case"], str(tmp_path / n))
        code = run_product(emu_engine_factory(), ["-i", inp, "-o", out] + g["case"]["argv"])
        assert code == g["case"]["exit"]
        compare_replayed(g["expected"], cli_cases.normalise(out), n)


@pytest.mark.gpu
def test_cli_golden_cases_on_gpu(gold_dir, tmp_path):
    """The same recorded runs of the reference's main() through the real CLI on the MI355X (fresh contexts, the native reader)."""
    names = golden_cases(gold_dir)
    assert len(names) >= 5
    for n in names:
        g = json.load(open(os.path.join(gold_dir, n)))
        inp, out = cli_cases.materialise(g["case"], str(tmp_path / n))
        try:
            cli.main(["-i", inp, "-o", out] + g["case"]["argv"])
            code = None
        except SystemExit as e:
            code = e.code if e.code is not None else 0
        assert code == g["case"]["exit"]
        compare_replayed(g["expected"], cli_cases.normalise(out), n)


def _dup_file(tmp_path):
    fa = tmp_path / "dups.fasta"
    return str(fa), cli_cases.write_duplicate_ids_fasta(str(fa))


def test_duplicate_read_ids_per_read_api_like_upstream(tmp_path, recorded):
    """Two records with one id (malformed input).  Upstream's bound_detect has no `break` and overwrites maxlengthtelo with the
    first matching record's length when that is shorter (allsteps.py:257-264): the second record is clipped by the shortest
    record before it.  The per-read API reproduces that (6 of 6 fuzz differences were this)."""
    from emu_engine import EmuEngine
    from topsicle_amd import allsteps
    fa, _ = _dup_file(tmp_path)
    calls = recorded["duplicate_ids"]
    assert [(c["tail"], c["maxlen"]) for c in calls] == cli_cases.DUP_BOUND_CALLS
    allsteps.set_engine(EmuEngine())
    try:
        for c in calls:
            tail, M = c["tail"], c["maxlen"]
            got = allsteps.bound_detect(fa, "dup", "CCCTAA", 100, 6, 100, M, 4, tail=tail)
            assert [list(r) for r in got] == c["want"], (tail, M)
            assert len(got) == (4 if tail is None else 2)
    finally:
        allsteps.set_engine(None)


def test_duplicate_read_ids_in_the_batched_cli_are_records_of_their_own(tmp_path, emu_engine_factory):
    """DELIBERATE DEVIATION: upstream's CLI looks every passing id up again in the filtered file and takes
    `bound_res[0]` -- with duplicate ids BOTH rows get the FIRST record's boundary, computed with the LAST record's tail
    (main.py:60, 125-133; allsteps.py:257-297).  The batched CLI reports every record by its own sequence and tail."""
    import csv
    import topsicle_oracle as orc
    fa, seqs = _dup_file(tmp_path)
    out = tmp_path / "o"
    assert run_product(emu_engine_factory(), ["-i", fa, "-o", str(out), "--pattern", "CCCTAA", "--minSeqLength", "1000", "--cutoff", "0.3"]) is None
    rows = list(csv.reader(open(out / "telolengths_all.csv")))[1:]
    assert [r[3] for r in rows] == ["dup", "solo", "dup"]
    pats = orc.kmer_table("CCCTAA", 4)
    for r, key in zip(rows, ("b", "a", "c")):
        cs, ce = orc.trc_counts(seqs[key], pats)
        call = orc.trc_call(cs, ce, pats, 6, 0.3)
        assert f"{call[2]:.3f}" == r[2]
        assert orc.step2(seqs[key], call[1], pats, 100, 6, 100, 20000) == int(r[4])
