"""BAM input on the MI355X: tps_batch_upload_nib4 (BAM's 4-bit codes expanded on the device) leaves the same packed batch as the
ASCII upload of the same reads, its scans give the same results, and the CLI on BAM gives what it gives on the FASTQ of the same
records."""
import csv
import os
import random

import numpy as np
import pytest

import bam_tools as bt
from topsicle_amd import hiplib, main as cli, seqio

pytestmark = pytest.mark.gpu

NT16 = bt.NT16


def _nib4_batch(reads, align_extra=0):
    """(nib, src, desc, n_words, ascii reads) for reads = [(stored codes as letters, reverse)]: the layout tps_reader_next_nib4 gives."""
    nib, src, ascii_reads = [], [], []
    off = 0
    for s, rev in reads:
        L = len(s)
        codes = [bt.CODE[c] for c in s] + ([0] if L & 1 else [])
        b = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))
        pad = ((len(b) + 15) // 16) * 16 + align_extra
        nib.append(b + bytes(pad - len(b)))
        src.append((off, hiplib.NIB_REVERSE if rev else 0, 0))
        off += pad
        ascii_reads.append(bt.revcomp(s) if rev else s)
    nib = np.frombuffer(b"".join(nib), np.uint8).copy() if nib else np.zeros(0, np.uint8)
    src = np.array(src, hiplib.NIB_SRC_DTYPE)
    bases, offsets = hiplib.pack_reads(ascii_reads)
    seq2, inv, desc = seqio.pack_reads_host(bases, offsets)
    return nib, src, desc.copy(), len(seq2), ascii_reads


def _reads(seed, lengths, iupac=True):
    rng = random.Random(seed)
    out = []
    for i, L in enumerate(lengths):
        alpha = "ACGT" if not iupac or i % 3 else NT16
        s = "".join(rng.choice(alpha) for _ in range(L))
        out.append((s, bool(i % 2)))
    return out


LENGTHS = [0, 1, 2, 3] + [b + d for b in (16, 32, 48, 64, 128, 192) for d in (-2, -1, 0, 1, 2)] + [500, 999, 4097, 15000, 69_999, 70_000]


@pytest.fixture(scope="module")
def sc():
    s = hiplib.HipScanner(0)
    yield s
    s.close()


@pytest.mark.parametrize("pinned", [False, True])
def test_nib4_upload_layout_equals_ascii_upload(sc, pinned):
    reads = _reads(1, LENGTHS) + _reads(2, [17, 33, 65, 129, 31, 63, 15], iupac=False)
    nib, src, desc, nw, ascii_reads = _nib4_batch(reads)
    if pinned:
        buf = sc.host_alloc(len(nib) + 16 * len(src) + 16 * len(desc) + 64)
        pn = buf[:len(nib)]
        pn[:] = nib
        ps = buf[len(nib):len(nib) + 16 * len(src)].view(hiplib.NIB_SRC_DTYPE)
        ps[:] = src
        pd = buf[len(nib) + 16 * len(src):len(nib) + 16 * len(src) + 16 * len(desc)].view(hiplib.DESC_DTYPE)
        pd[:] = desc
        nib, src, desc = pn, ps, pd
    sc.upload_nib4(3, nib, src, desc, nw)
    sc.sync()
    got = sc.download_packed(3)
    bases, offsets = hiplib.pack_reads(ascii_reads)
    sc.upload(4, bases, offsets)
    want = sc.download_packed(4)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    if pinned:
        sc.host_free(buf)


def test_nib4_slots_and_reverse_every_residue(sc):
    """Every residue of the length mod 64 in both orientations, over several slots at once."""
    for slot, seed in ((0, 5), (1, 6), (2, 7)):
        lengths = [64 * (seed - 4) + r for r in range(0, 130)]
        reads = _reads(seed, lengths)
        reads = [(s, (i + seed) % 2 == 0) for i, (s, _) in enumerate(reads)]
        nib, src, desc, nw, ascii_reads = _nib4_batch(reads)
        sc.upload_nib4(slot, nib, src, desc, nw)
        bases, offsets = hiplib.pack_reads(ascii_reads)
        sc.upload(5 + slot, bases, offsets)
    sc.sync()
    for slot in range(3):
        for g, w in zip(sc.download_packed(slot), sc.download_packed(5 + slot)):
            assert np.array_equal(g, w)


def test_nib4_rejects_codes_outside_the_buffer(sc):
    reads = _reads(9, [100, 200])
    nib, src, desc, nw, _ = _nib4_batch(reads)
    bad = src.copy()
    bad["off"][1] = len(nib)                                # past the end
    with pytest.raises(hiplib.TopsicleHipError):
        sc.upload_nib4(8, nib, bad, desc, nw)
    bad = src.copy()
    bad["off"][1] += 8                                     # not on a 16-byte boundary
    with pytest.raises(hiplib.TopsicleHipError):
        sc.upload_nib4(8, np.concatenate([nib, np.zeros(16, np.uint8)]), bad, desc, nw)


def test_nib4_scan_equals_packed_scan(sc, tmp_path):
    """A BAM file's nib4 batches, scanned: results, window sums and raw rows equal those of the host-packed upload."""
    path = str(tmp_path / "r.bam")
    bt.write_bam(path, bt.make_reads(seed=21, n=120, lengths=[3000 + 37 * i for i in range(40)]), block=20000)
    pats = ["CCCTA", "CCTAA", "CTAAA", "TAAAC", "AAACC", "AACCC", "ACCCT", "TAGGG", "TTAGG", "TTTAG", "GTTTA", "GGTTT", "GGGTT", "AGGGT"]
    sc.set_patterns(pats)
    prm = hiplib.make_params(min_len=1000, min_count=10, window=100, slide=6, trimfirst=100, maxlen=20000,
                             flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG | hiplib.F_STORE_SUMS | hiplib.F_STORE_RAW)
    pool = seqio.BufferPool(2, 1 << 16, 64, sc.host_alloc)
    n = 0
    for pb in seqio.read_batches_packed(path, pool, max_records=64):
        sc.upload_nib4(0, pb.nib, pb.src, pb.desc, pb.n_words)
        seq2, inv, desc = seqio.pack_nib4_host(pb.nib, pb.src, pb.desc, pb.n_words)
        sc.upload_packed(1, seq2, inv if (desc["flags"] & 1).any() else None, desc)
        outs = []
        for slot in (0, 1):
            sc.scan(slot, prm)
            sc.sync()
            outs.append((sc.results(slot), sc.window_sums(slot), sc.window_raw(slot)))
        (r0, s0, w0), (r1, s1, w1) = outs
        assert np.array_equal(r0, r1) and r0["pass"].sum() > 0
        assert np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1])
        assert np.array_equal(w0[0], w1[0])
        n += pb.n
        pb.release()
    assert n > 50


def _cli(argv, engines=None):
    args = cli.build_parser().parse_args(argv)
    cli.tprint.logfile = cli.get_log_path(args)
    cli.analysis_run(args, engines=engines)


def _rows(path):
    return [r[1:] for r in csv.reader(open(path))]


def test_gpu_cli_demo_ubam_and_same_records(tmp_path, gold_dir):
    d = tmp_path / "in"
    d.mkdir()
    bt.fastq_records_to_bam(os.path.join(gold_dir, "demo_col0.fastq.gz"), str(d / "Col-0-6909_GWHBDNP00000001.1_nano_right.bam"))
    out = tmp_path / "demo"
    _cli(["-i", str(d), "-o", str(out), "--pattern", "CCCTAAA", "--slide", "6", "--gpus", "1"])
    assert _rows(out / "telolengths_all.csv") == _rows(os.path.join(gold_dir, "demo_telolengths_all.csv"))
    # a BAM and the FASTQ of its records, three k at once (contexts share the batch), raw rows as CSV and npz
    from test_bam_input import _same_records
    bam, fq = _same_records(tmp_path)
    for fmt in ("csv", "npz"):
        res = {}
        for name, path in (("bam", bam), ("fq", fq)):
            o = tmp_path / f"{fmt}_{name}"
            _cli(["-i", path, "-o", str(o), "--pattern", "CCCTAAA", "--slide", "6", "--telophrase", "4", "5", "6", "--rawcountpattern",
                  "--rawcountformat", fmt, "--cutoff", "0.4", "--gpus", "1"])
            res[name] = o
        a, b = res["bam"], res["fq"]
        assert _rows(a / "telolengths_all.csv") == _rows(b / "telolengths_all.csv")
        assert open(a / "sample_trc_over_0.4.fastq", "rb").read() == open(b / "sample_trc_over_0.4.fastq", "rb").read()
        files = sorted(f for f in os.listdir(a) if f.startswith("rawcount_"))
        assert files and files == sorted(f for f in os.listdir(b) if f.startswith("rawcount_"))
        for f in files:
            if fmt == "csv":
                assert open(a / f, "rb").read() == open(b / f, "rb").read(), f
            else:
                za, zb = np.load(a / f), np.load(b / f)
                for key in za.files:
                    assert np.array_equal(za[key], zb[key]), (f, key)
