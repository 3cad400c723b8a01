"""BAM input without a GPU: the native reader against an independent decoder (what `samtools fastq` gives), the host nib4 packer
against the ASCII packer, the filtered-FASTQ writer, loud errors, and the whole CLI on emulated engines (BAM and the FASTQ of the
same records give the same outputs)."""
import csv
import os
import shutil
import struct

import numpy as np
import pytest

import bam_tools as bt
from topsicle_amd import main as cli, seqio


@pytest.fixture()
def io_defaults():
    yield
    for k, v in seqio.IO_OPTION_DEFAULTS.items():
        seqio.io_option(k, v)


def _ascii_records(path):
    out = []
    for b in seqio.read_batches(path, max_bases=1 << 18, max_records=7):
        for i in range(b.n):
            r = b.record(i)
            out.append((r.id, r.seq, r.qual))
    return out


def _nib_batches(path, words_cap=8192, reads_cap=9):
    pool = seqio.BufferPool(2, words_cap, reads_cap)
    for pb in seqio.read_batches_packed(path, pool, max_records=reads_cap):
        yield pb
        pb.release()


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("group", [0, 40_000, 7_000])
def test_reader_ascii_batches_equal_decode(tmp_path, io_defaults, aligned, group):
    """uBAM and aligned BAM: reverse / secondary / supplementary records, l_seq = 0, odd lengths, IUPAC and '=' bases, missing
    qualities, records larger than a BGZF block; small blocks and refill windows make records straddle both."""
    path = str(tmp_path / "reads.bam")
    bt.write_bam(path, bt.make_reads(seed=3 + aligned, aligned=aligned), block=5000 if group else 65280)
    seqio.io_option("bgzf_group", group)
    want = bt.decode_bam(path)
    assert len(want) > 20 and any(len(s) == 0 for _, s, _ in want) and any("=" in s for _, s, _ in want)
    assert seqio.is_bam(path)
    got = _ascii_records(path)
    assert got == want
    assert [(r.id, r.seq, r.qual) for r in seqio.read_records(path)] == want


def test_reader_format_code_and_refusals(tmp_path):
    import ctypes as C
    path = str(tmp_path / "r.bam")
    bt.write_bam(path, bt.make_reads(n=5))
    lib = seqio._load_io()
    h = C.c_void_p()
    assert lib.tps_reader_open(path.encode(), C.byref(h)) == 0
    try:
        assert lib.tps_reader_format(h) == 3
        nw = C.c_int64(0)
        seq2, inv = np.zeros(1 << 16, np.uint32), np.zeros(1 << 16, np.uint16)
        desc = np.zeros(64, np.uint8)
        heads, ho, spans = np.zeros(1 << 16, np.uint8), np.zeros(8, np.int64), np.zeros(32, np.int64)
        assert lib.tps_reader_next_packed(h, seq2.ctypes.data, inv.ctypes.data, 1 << 16, desc.ctypes.data, 4, heads.ctypes.data, len(heads),
                                          ho.ctypes.data, spans.ctypes.data, C.byref(nw)) == -1
        assert b"nib4" in lib.tps_io_last_error()
    finally:
        lib.tps_reader_close(h)
    h2 = C.c_void_p()
    assert lib.tps_reader_open_range(path.encode(), 0, 100, 0, C.byref(h2)) == -1


@pytest.mark.parametrize("group", [0, 9_000])
def test_nib4_batches_pack_like_ascii(tmp_path, io_defaults, group):
    """tps_pack_nib4 of every nib4 batch equals tps_pack_reads of the decoded ASCII of the same records, bit for bit; the reader's
    descriptors (layout and TPS_RD_HAS_INVALID) are the packer's."""
    path = str(tmp_path / "reads.bam")
    bt.write_bam(path, bt.make_reads(seed=5, n=80), block=3000)
    seqio.io_option("bgzf_group", group)
    want = bt.decode_bam(path)
    k = 0
    n_batches = 0
    for pb in _nib_batches(path, words_cap=8192, reads_cap=9):
        n_batches += 1
        assert pb.fmt == "bam" and pb.seq2 is None and pb.nib is not None
        assert np.all(pb.src["off"] % 16 == 0)
        recs = want[k:k + pb.n]
        k += pb.n
        assert pb.ids == [r[0] for r in recs]
        seq2, inv, desc = seqio.pack_nib4_host(pb.nib, pb.src, pb.desc, pb.n_words)
        bases = np.frombuffer("".join(r[1] for r in recs).encode(), np.uint8)
        offsets = np.concatenate([[0], np.cumsum([len(r[1]) for r in recs])]).astype(np.int64)
        s2, i2, d2 = seqio.pack_reads_host(bases, offsets)
        assert np.array_equal(seq2, s2) and np.array_equal(inv, i2) and np.array_equal(desc, d2)
        assert np.array_equal(pb.desc, d2)
        assert pb.n_words == len(s2)
        assert [pb.seq_bytes(i).decode() for i in range(pb.n)] == [r[1] for r in recs]
        assert [pb.qual_bytes(i).decode() for i in range(pb.n)] == [r[2] for r in recs]
    assert k == len(want) and n_batches > 3


def test_filtered_fastq_writer(tmp_path, io_defaults):
    path = str(tmp_path / "reads.bam")
    bt.write_bam(path, bt.make_reads(seed=7, n=50), block=4000)
    seqio.io_option("bgzf_group", 20_000)
    want = bt.decode_bam(path)
    out = tmp_path / "out.fastq"
    expect = []
    k = 0
    with open(out, "wb") as fh:
        off = 0
        for pb in _nib_batches(path, words_cap=8192, reads_cap=6):
            recs = want[k:k + pb.n]
            k += pb.n
            idx = np.arange(pb.n)[::2]
            nbytes = pb.native_fastq_bytes(idx, "fastq")
            lib = seqio._load_io()
            lens = np.ascontiguousarray(pb.desc["len"], np.int32)
            spans = np.ascontiguousarray(pb.spans, np.int64)
            assert nbytes == lib.tps_fastq_spans_bytes(spans.ctypes.data, lens.ctypes.data, np.ascontiguousarray(idx, np.int64).ctypes.data, len(idx))
            pb.write_records(fh, idx, "fastq", offset=off)
            off += nbytes
            chunk = "".join(f"@{recs[i][0]}\n{recs[i][1]}\n+\n{recs[i][2]}\n" for i in idx).encode()
            assert len(chunk) == nbytes
            expect.append(chunk)
    assert open(out, "rb").read() == b"".join(expect)
    # without an offset: at the handle's position, the handle left behind what was written
    with open(tmp_path / "seq.fastq", "wb") as fh:
        for pb in _nib_batches(path):
            pb.write_records(fh, range(pb.n), "fastq")
    assert open(tmp_path / "seq.fastq", "rb").read() == "".join(f"@{n}\n{s}\n+\n{q}\n" for n, s, q in want).encode()


def _raw_bam_stream(reads):
    return bt.header_bytes() + b"".join(bt.record_bytes(n, f, s, q) for n, f, s, q in reads)


def _expect_error(path, match):
    with pytest.raises(RuntimeError, match=match):
        list(seqio.read_batches(path))
    with pytest.raises(RuntimeError, match=match):
        for pb in _nib_batches(path):
            pass


def test_damaged_files_are_loud_errors(tmp_path):
    reads = [("r%d" % i, 0, "ACGT" * (i + 1), "I" * 4 * (i + 1)) for i in range(30)]
    data = _raw_bam_stream(reads)
    # a record cut off at a block boundary (the file ends inside it; no EOF block)
    p = str(tmp_path / "cut.bam")
    with open(p, "wb") as fh:
        fh.write(bt.bgzf_block(data[:len(data) - 7]))
    _expect_error(p, "truncated")
    # a block cut in the middle
    full = bt.bgzf(data, block=300)
    p = str(tmp_path / "midblock.bam")
    with open(p, "wb") as fh:
        fh.write(full[:len(full) // 2])
    _expect_error(p, "BGZF|truncated")
    # a block_size that runs past the data
    bad = bytearray(data)
    first = len(bt.header_bytes())
    struct.pack_into("<i", bad, first + 4 * 0, 10_000_000)
    p = str(tmp_path / "overlong.bam")
    with open(p, "wb") as fh:
        fh.write(bt.bgzf(bytes(bad)))
    _expect_error(p, "truncated")
    # fields that run past the record's block_size
    bad = bytearray(data)
    struct.pack_into("<i", bad, first + 4 + 16, 5000)          # l_seq
    p = str(tmp_path / "fields.bam")
    with open(p, "wb") as fh:
        fh.write(bt.bgzf(bytes(bad)))
    _expect_error(p, "block_size")
    # block_size below the fixed fields
    bad = bytearray(data)
    struct.pack_into("<i", bad, first, 12)
    p = str(tmp_path / "small.bam")
    with open(p, "wb") as fh:
        fh.write(bt.bgzf(bytes(bad)))
    _expect_error(p, "block_size")
    # bad magic: not BAM, not FASTA / FASTQ -> refused at open
    p = str(tmp_path / "magic.bam")
    with open(p, "wb") as fh:
        fh.write(bt.bgzf(b"BAX\x01" + data[4:]))
    assert not seqio.is_bam(p)
    assert list(seqio.read_batches(p)) == []
    import ctypes as C
    lib = seqio._load_io()
    h = C.c_void_p()
    assert lib.tps_reader_open(p.encode(), C.byref(h)) == -1 and b"format" in lib.tps_io_last_error()
    # a header that ends early
    p = str(tmp_path / "head.bam")
    with open(p, "wb") as fh:
        fh.write(bt.bgzf(bt.header_bytes()[:30]))
    _expect_error(p, "header")


# ------------------------------------------------------------------------------------------------ whole CLI, emulated engines
def run_cli(engine, argv):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=[engine] if engine is not None else None)
    return args


def _csv_rows(path, drop_file=True):
    rows = list(csv.reader(open(path)))
    return [r[1:] for r in rows] if drop_file else rows


def test_cli_demo_as_ubam_reproduces_reference_rows(tmp_path, gold_dir):
    d = tmp_path / "in"
    d.mkdir()
    bam = str(d / "Col-0-6909_GWHBDNP00000001.1_nano_right.bam")
    reads = bt.fastq_records_to_bam(os.path.join(gold_dir, "demo_col0.fastq.gz"), bam, block=20000)
    out = tmp_path / "out"
    run_cli(bt.NibEmuEngine(), ["--inputDir", str(d), "--outputDir", str(out), "--pattern", "CCCTAAA", "--slide", "6"])
    got = _csv_rows(out / "telolengths_all.csv")
    want = _csv_rows(os.path.join(gold_dir, "demo_telolengths_all.csv"))
    assert got == want and len(got) > 10
    assert all(r[0] == "Col-0-6909_GWHBDNP00000001.1_nano_right" for r in _csv_rows(out / "telolengths_all.csv", False)[1:])
    filt = out / "Col-0-6909_GWHBDNP00000001.1_nano_right_trc_over_0.7.fastq"
    byid = {r[0]: r for r in reads}
    recs = list(seqio.read_records(str(filt)))
    assert [r.id for r in recs] == [w[2] for w in want[1:]]
    assert all(r.seq == byid[r.id][2] and r.qual == byid[r.id][3] for r in recs)


def _same_records(tmp_path, seed=11):
    """A BAM of telomeric and other reads (reverse ones among them), and the FASTQ of what its decode gives."""
    d_bam, d_fq = tmp_path / "bam", tmp_path / "fq"
    d_bam.mkdir()
    d_fq.mkdir()
    import random
    rng = random.Random(seed)
    reads = []
    for i in range(40):
        L = rng.randint(3000, 12000)
        tract = rng.randint(400, 2500) if i % 4 else 0
        body = "".join(rng.choice("ACGT") for _ in range(L - tract))
        s = ("CCCTAAA" * (tract // 7 + 1))[:tract] + body if i % 2 else body + ("TTTAGGG" * (tract // 7 + 1))[:tract]
        if i % 5 == 0:
            s = s[:100] + "N" + s[101:]
        flag = [0, bt.FLAG_REVERSE, bt.FLAG_UNMAPPED, bt.FLAG_SECONDARY, bt.FLAG_REVERSE | bt.FLAG_SUPPLEMENTARY][i % 5]
        q = "".join(chr(33 + rng.randint(0, 40)) for _ in range(L))
        reads.append((f"read_{i}", flag, s, q, [(L, "M")] if flag != bt.FLAG_UNMAPPED else [], [("RG", "Z", "x")]))
    bam = str(d_bam / "sample.bam")
    bt.write_bam(bam, reads, block=30000)
    fq = str(d_fq / "sample.fastq")
    bt.write_fastq(fq, bt.decode_bam(bam))
    return bam, fq


@pytest.mark.parametrize("fmt", ["csv", "npz"])
def test_cli_bam_and_fastq_of_same_records_agree(tmp_path, fmt):
    bam, fq = _same_records(tmp_path)
    outs = {}
    for name, path in (("bam", bam), ("fq", fq)):
        out = tmp_path / f"out_{name}"
        run_cli(bt.NibEmuEngine(), ["-i", path, "-o", str(out), "--pattern", "CCCTAAA", "--slide", "6", "--telophrase", "4", "5", "6",
                                    "--rawcountpattern", "--rawcountformat", fmt, "--cutoff", "0.4"])
        outs[name] = out
    a, b = outs["bam"], outs["fq"]
    rows = _csv_rows(a / "telolengths_all.csv")
    assert rows == _csv_rows(b / "telolengths_all.csv") and len(rows) > 10
    assert open(a / "sample_trc_over_0.4.fastq", "rb").read() == open(b / "sample_trc_over_0.4.fastq", "rb").read()
    log_a = [ln.split("] ", 1)[-1] for ln in open(a / "topsicle_run.log").read().splitlines()]
    log_b = [ln.split("] ", 1)[-1] for ln in open(b / "topsicle_run.log").read().splitlines()]
    summary = [ln for ln in log_b if "median" in ln.lower() or "asymptotic" in ln.lower()]
    assert summary and all(ln in log_a for ln in summary)
    raw_a = sorted(f for f in os.listdir(a) if f.startswith("rawcount_"))
    assert raw_a == sorted(f for f in os.listdir(b) if f.startswith("rawcount_")) and raw_a
    for f in raw_a:
        if fmt == "csv":
            assert open(a / f, "rb").read() == open(b / f, "rb").read(), f
        else:
            za, zb = np.load(a / f), np.load(b / f)
            assert sorted(za.files) == sorted(zb.files)
            for key in za.files:
                assert np.array_equal(za[key], zb[key]), (f, key)


def test_cli_folder_with_bam_and_flags_resolved(tmp_path):
    bam, fq = _same_records(tmp_path, seed=13)
    folder = tmp_path / "mixed"
    folder.mkdir()
    shutil.copy(bam, folder / "a.bam")
    out = tmp_path / "out"
    run_cli(bt.NibEmuEngine(), ["-i", str(folder), "-o", str(out), "--pattern", "CCCTAAA", "--slide", "6", "--cutoff", "0.4",
                                "--twopass", "on", "--shards", "4"])
    rows = _csv_rows(out / "telolengths_all.csv", drop_file=False)
    assert len(rows) > 5 and {r[0] for r in rows[1:]} == {"a"}
    log = open(out / "topsicle_run.log").read()
    assert "--twopass on ignored" in log and "--shards 4 ignored" in log
    assert os.path.exists(out / "a_trc_over_0.4.fastq")


def test_allsteps_file_functions_take_bam(tmp_path):
    from topsicle_amd import allsteps
    bam, fq = _same_records(tmp_path, seed=17)
    assert seqio.check_file_type(bam) == "bam" and seqio.check_file_type(fq) == "fastq"
    eng = bt.NibEmuEngine()
    allsteps.set_engine(eng)
    try:
        a = allsteps.patternTRC_count(bam, "CCCTAAA", read_length=1000, kmer=5, no_bp=1000, cutoff=0.4)
        b = allsteps.patternTRC_count(fq, "CCCTAAA", read_length=1000, kmer=5, no_bp=1000, cutoff=0.4)
        assert a == b and len(a) > 3
        rid = bt.decode_bam(bam)[1][0]
        pats = allsteps.patterns_to_search("CCCTAAA", 5)
        assert allsteps.bound_detect(bam, rid, pats, 100, 6, 100, 20000, 5) == allsteps.bound_detect(fq, rid, pats, 100, 6, 100, 20000, 5)
    finally:
        allsteps.set_engine(None)
