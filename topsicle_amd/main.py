"""`topsicle` command line on MI355X: same flags, output files and log lines as the reference's
Topsicle/main.py (flags main.py:319-334; CSV header :200, rows :138; log lines :266, 293, 302,
309), with the per-read work done in batched HIP launches instead of the reference's
one-process-per-file pool and per-read file re-parsing (main.py:125-152, 232-235).

Extra flags (not in the reference): --gpus N shards batches of reads over N GPUs of the node
(one host thread + one context per GPU, no collective); --device picks the first GPU.
"""
from __future__ import annotations

import argparse
import csv
import datetime
import os
import queue
import sys
import threading
import time
from collections import defaultdict

import numpy as np

from . import adapters, allsteps, anchor, batch, consensus, endref, ends, hiplib, methyl, motif, rawnpz, refine, seqio, tracts, variants

version_number = "1.0.0"
Topsicle_output_prefix = "Topsicle"
CONTEXTS_PER_GPU = 2
WRITER_THREADS = 1                # threads that write the passing records (native FASTQ writer, pwritev at offsets known up front).  Three were measured
                                  # (round 5, configs[3]'s shard: 7.5 GB of records): buffered writes into ONE file serialise on the inode, three threads
                                  # reach 1.4 - 2.0 GB/s each where one reaches 4.9 - 6.5 -- 1.68 -> 2.30 s (.gz), 1.50 -> 2.07 s (BGZF); one it is
# The read analyses, in the order of their launches behind a scan and of their blocks in the log.  Each module has the CLI's side of
# its analysis: FLAG (the flag that turns it on = its keyword of batch.Job), cli_check(args, root) -> None or the words after
# "--flag needs", POWER_NOTE (what it does with a motif that is a power of its root), cli_collector(args, unit, slide),
# Collector.keep_row (what is kept per read with a stored boundary) and finish_and_write(args, k, col, filenames, engines) -> log lines.
PER_K_ANALYSES = (variants, ends, adapters, refine, methyl)       # one collector per k
ANALYSES = PER_K_ANALYSES + (tracts,)                     # one for the run: the map of whole reads, with the first k's job
# ... and what is checked before anything is read or written, in this order (--variants is only checked against the real unit;
# --anchor and --endref hang on --ends and have nothing else to check)
EARLY_CHECKS = (tracts, ends, anchor, consensus, endref, adapters, refine, methyl)
LAST_TIMINGS = {}                 # seconds of the last analysis_run: reads (step 1 + 2 + outputs) / summary (fit + PNG); bench.py's e2e leg reads it
PLOT_THREADS = []                 # quadratic-fit PNGs being rendered off the critical path (summarize); wait_for_plots() joins them


def wait_for_plots():
    """Block until every summary PNG of earlier runs is on disk; an exception inside a drawing is reported here (it used to
    be lost in its thread and a missing quadfit_*.png went unnoticed)."""
    _PLOT_JOBS.join()
    errs, PLOT_ERRORS[:] = list(PLOT_ERRORS), []
    for path, err in errs:
        tprint(f"summary plot {path} failed: {err!r}")
    return errs


# The summary pictures are drawn by ONE worker thread, one after the other (one thread per k-mer length rendered them
# concurrently -- Agg rendering with shared font caches is only safe on recent matplotlib)
import queue as _queue  # noqa: E402

_PLOT_JOBS: "_queue.Queue" = _queue.Queue()
PLOT_ERRORS: list = []


def _plot_worker():
    while True:
        fn, fargs, path = _PLOT_JOBS.get()
        try:
            fn(*fargs)
        except BaseException as e:                                   # reported by wait_for_plots()
            PLOT_ERRORS.append((path, e))
        finally:
            _PLOT_JOBS.task_done()


def _submit_plot(fn, fargs, path):
    if not PLOT_THREADS:                       # the one worker, started with the first picture; a process that ends waits for its queue
        import atexit
        t = threading.Thread(target=_plot_worker, daemon=True)
        t.start()
        PLOT_THREADS.append(t)
        atexit.register(wait_for_plots)
    _PLOT_JOBS.put((fn, fargs, path))


def warm_up_plotting():
    """Import matplotlib's Agg machinery on a helper thread while the reads are being scanned (the import costs more than the
    drawing): by the time the summary wants its PNG the modules are there."""
    def imp():
        try:
            from matplotlib.backends.backend_agg import FigureCanvasAgg  # noqa: F401
            from matplotlib.figure import Figure  # noqa: F401
        except Exception:
            pass
    t = threading.Thread(target=imp, daemon=True)
    t.start()
    return t


def get_log_path(args):
    log_dir = getattr(args, "outputDir", ".")
    os.makedirs(log_dir, exist_ok=True)
    return os.path.join(log_dir, "topsicle_run.log")


def tprint(*args, **kwargs):
    """Timestamped print, mirrored into <outputDir>/topsicle_run.log (main.py:37-45)."""
    msg = " ".join(str(a) for a in args)
    now = datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S")
    line = f"[{now}] {msg}"
    print(line)
    if hasattr(tprint, "logfile"):
        with open(tprint.logfile, "a") as f:
            f.write(line + "\n")


def _formats(seq_loc: str):
    """(input format, filtered-file extension) by file name, as main.py:68-81 decides it; BAM input (recognised by its content)
    leaves its passing records as FASTQ."""
    if seqio.is_bam(seq_loc):
        return "fastq"
    if seq_loc.endswith(".gz"):
        fq = seq_loc.endswith(".fastq.gz") or seq_loc.endswith(".fq.gz")
    else:
        fq = seq_loc.endswith(".fastq") or seq_loc.endswith(".fq")
    return "fastq" if fq else "fasta"


_CSV_LOCK = __import__("threading").Lock()      # telolengths_all.csv is appended batch by batch from every file in flight


NO_BP = 1000                                    # bases of a read end that step 1 counts in (main.py:52-60)


def _scan_params(args, slide):
    """The parameters of one k's scan: of the reads of every input file, and of the pieces of --endref."""
    min_cutoff = min(args.cutoff) if isinstance(args.cutoff, (list, tuple)) else args.cutoff
    return hiplib.make_params(
        no_bp=NO_BP, min_len=args.minSeqLength, min_count=allsteps.min_count_for_cutoff(min_cutoff, NO_BP / len(args.pattern), NO_BP),
        window=args.windowSize, slide=slide, trimfirst=args.trimfirst, maxlen=args.maxlengthtelo,
        flags=hiplib.F_STEP1 | hiplib.F_WINDOWS | hiplib.F_BINSEG)


def process_file(args, seq_loc, telo_phrase, pattern, sliding_val, engines):
    """One input file, one k (main.py:52-154).  Returns [(file_name, telo_phrase, [[readID, telolen]], trc), ...] in read order."""
    return process_file_multi(args, seq_loc, [(telo_phrase, pattern, sliding_val)], engines)[0]


def process_file_multi(args, seq_loc, phrases, engines):
    """One input file, every requested k in ONE pass: each batch is parsed, packed and uploaded once and scanned once per
    k-mer table (`phrases` = [(telo_phrase, pattern list, slide), ...]).  Per k it does what the reference's process_file
    does (main.py:52-154): step 1 + filtered file + step 2 rows; the per-read work of a batch is numpy arithmetic on the
    kernel's result records, one bulk write of the passing records and one bulk CSV append.  Rows of the first k are
    appended to telolengths_all.csv batch by batch; the other k's rows are returned for the caller to append behind them
    (the reference writes all rows of one k before the next).  Returns one row list per k:
    [(file_name, telo_phrase, [[readID, telolen]], trc), ...] in read order."""
    tprint("subsetting raw dataset based on TRC cutoff")
    base_name = os.path.basename(seq_loc)
    file_name = os.path.splitext(base_name)[0]
    min_cutoff = min(args.cutoff) if isinstance(args.cutoff, (list, tuple)) else args.cutoff
    no_bp = NO_BP
    ratio = no_bp / len(args.pattern)
    want_sums = bool(args.plot)
    want_raw = bool(args.rawcountpattern)
    # --rawcountformat npz: one archive per input file and k, its rows written device -> file by the batch workers (rawnpz.py)
    npz = want_raw and getattr(args, "rawcountformat", "csv") == "npz"
    raw_npz = [rawnpz.RawNpzWriter(f"{args.outputDir}/rawcount_{telo_phrase}_{file_name}.npz", pattern, sliding_val, args.read_check or None)
               if npz else None for telo_phrase, pattern, sliding_val in phrases]
    # the read analyses: per k {flag: collector} for the whole run (analysis_run made them); the kernels run on the batch workers
    cols = getattr(args, "analysis_collectors", None) or [{} for _ in phrases]
    jobs = [batch.Job(pattern, _scan_params(args, slide), want_sums, want_raw, raw_sink=sink, **{flag: col.spec for flag, col in mine.items()})
            for (_k, pattern, slide), sink, mine in zip(phrases, raw_npz, cols)]
    # --tracts: one collector for the whole run; the map runs once per batch, with the first k's job
    tcol = getattr(args, "tract_collector", None)
    if tcol is not None:
        jobs[0].tracts = tcol.spec

    fmt = _formats(seq_loc)
    fasta_temp = os.path.join(args.outputDir, f"{file_name}_trc_over_{min_cutoff}.fasta")
    out_handle = None
    if os.path.exists(fasta_temp):
        tprint(f"Temporary fasta file already exists: {fasta_temp}. Using existing file.")
    else:
        fasta_temp = os.path.join(args.outputDir, f"{file_name}_trc_over_{min_cutoff}.{fmt}")
        out_handle = open(fasta_temp, "wb")
    # Which k's passing records the file holds after upstream's OUTER loop over k (main.py:206-235, 64-78): FASTA input -- the
    # first k writes <name>.fasta, every later k finds it and reuses it, so the FIRST k's records stay; FASTQ input -- only
    # `.fasta` is ever checked, the `.fastq` file is rewritten for every k, so the LAST k's records stay.
    writer_k = 0 if fmt == "fasta" else len(phrases) - 1

    rows = [[] for _ in phrases]
    image_num = [1] * len(phrases)
    csv_path = f"{args.outputDir}/telolengths_all.csv"
    pool = batch.EnginePool(engines, two_pass=getattr(args, "twopass", None))
    # the passing records are written by a helper thread while the next batches are scanned (the native writer releases the GIL:
    # pwritev straight from the mapped input).  Round 5: every batch whose records leave through the native writer gets its place in
    # the file up front (a record takes header + 2 x bases + 6 bytes), so the writes need no order -- several threads could write
    # different batches at once; measured, they do not pay (WRITER_THREADS above).  BASELINE configs[3]'s shard rewrites 7.5 GB: that
    # one thread at 5 - 6 GB/s is what the run waits for.  Batches of other kinds (FASTA, ASCII batches) are written in order, after
    # everything before them has landed.
    wq: "queue.Queue" = queue.Queue(maxsize=2 * WRITER_THREADS + 2)
    werr = []
    wstat = {"write_s": 0.0, "blocked_s": 0.0, "records": 0}             # where the filtered file's time goes (logged below)
    wlock = threading.Lock()
    out_off = [0]                                                         # bytes of the filtered file given out so far

    def writer():
        while True:
            item = wq.get()
            try:
                if item is None:
                    return
                if not werr:
                    t0 = time.perf_counter()
                    item[0].write_records(out_handle, item[1], fmt, offset=item[2])
                    with wlock:
                        wstat["write_s"] += time.perf_counter() - t0
                        wstat["records"] += len(item[1])
            except BaseException as e:                                     # surfaces in the main thread below
                werr.append(e)
            finally:
                wq.task_done()
    wthreads = [threading.Thread(target=writer, daemon=True) for _ in range(WRITER_THREADS)] if out_handle is not None else []
    for t in wthreads:
        t.start()
    wthread = wthreads[0] if wthreads else None

    def write_passing(pb, idx):
        nbytes = pb.native_fastq_bytes(idx, fmt)
        t0 = time.perf_counter()
        if nbytes is not None:
            wq.put((pb, idx, out_off[0]))
            out_off[0] += nbytes
        else:
            wq.join()                                  # an ordered write: everything before it has landed
            out_handle.seek(out_off[0])
            pb.write_records(out_handle, idx, fmt)
            out_handle.flush()
            out_off[0] = out_handle.tell()
            wstat["records"] += len(idx)
        wstat["blocked_s"] += time.perf_counter() - t0

    # one big plain file on several GPUs: cut into byte ranges, a reader team per range (batch.EnginePool.scan_file_jobs; per-read
    # records only -- plots and raw rows keep one reader).  --shards N forces it (tests); the default cuts files of at least 256 MiB per GPU
    n_shards = int(getattr(args, "shards", 0) or 0)
    shard_min = 4096
    if seqio.is_bam(seq_loc):
        if n_shards > 1:
            tprint(f"{base_name}: BAM input is read by one reader (--shards {n_shards} ignored: BAM has no record index)")
        if getattr(args, "twopass", None) == "on":
            tprint(f"{base_name}: BAM input is scanned as whole reads (--twopass on ignored)")
    if n_shards <= 0:
        n_shards, shard_min = max(1, len({getattr(e, "device", 0) for e in engines})), 256 << 20
    ok = False
    try:
        for pb, outs in pool.scan_file_jobs(seq_loc, jobs, shards=n_shards, shard_min_bytes=shard_min):
            if tcol is not None:                                             # every read of the batch, passing or not
                t_tracts, t_found, _t_totals = tcol.take(pb)
                tcol.add_batch(seq_loc, file_name, lambda i: pb.read_id(int(i)), pb.desc["len"], t_tracts, t_found)
            for n, ((telo_phrase, pattern, sliding_val), (res, sums, raw, win_off)) in enumerate(zip(phrases, outs)):
                idx = np.nonzero(res["pass"])[0]
                taken = [(col, col.take_batch(pb)) for col in cols[n].values()]
                if wthread is not None and len(idx) and n == writer_k:
                    write_passing(pb, idx)                                   # every passing record (main.py:83-86)
                ids = [pb.read_id(int(i)) for i in idx]
                if args.read_check:
                    keep = [j for j, rid in enumerate(ids) if rid == args.read_check]
                    idx, ids = idx[keep], [ids[j] for j in keep]
                if not len(idx):
                    continue
                r = res[idx]
                fwd = r["tail"] == 0
                trc = np.where(fwd, r["best_start"], r["best_end"]) / ratio  # float64, like int / float upstream
                lens = pb.desc["len"][idx].astype(np.int64)
                m = np.minimum(args.maxlengthtelo, lens)
                bkp = r["bkp"].astype(np.int64)
                point = np.where(bkp >= 0, bkp * sliding_val + args.trimfirst, 0)
                telolen = np.where((point <= m) & (point != 0), point, 0)    # allsteps.py:330-333
                for j in np.nonzero(bkp < 0)[0]:
                    tprint(f"read {ids[j]}: {int(r['n_win'][j])} windows, no admissible change point; reporting 0")
                telo_l, trc_l = telolen.tolist(), trc.tolist()
                stored = np.nonzero(telolen != 0)[0]                         # one row per read with a stored boundary
                for col, out in taken:
                    col.add_file_rows(seq_loc, [col.keep_row(out, int(idx[j]), file_name, ids[j], int(r["tail"][j]), telo_l[j], int(lens[j])) for j in stored])
                if n == 0:
                    with _CSV_LOCK, open(csv_path, mode="a", newline="") as fh:
                        csv.writer(fh).writerows(zip([file_name] * len(ids), [telo_phrase] * len(ids), ["%.3f" % t for t in trc_l], ids, telo_l))
                rows[n] += [(file_name, telo_phrase, [[rid, tl]], t) for rid, tl, t in zip(ids, telo_l, trc_l)]
                if raw_npz[n] is not None:
                    # the rows are in the archive already (written by the worker that scanned the batch); what is kept here is
                    # one id, one tail and one window count per read -- no per-read loop over the rows
                    assert np.array_equal(raw.keep, idx)
                    raw_npz[n].add_reads(ids, np.where(fwd, "forward", "reverse").tolist(), r["n_win"])
                if args.plot or (args.rawcountpattern and raw_npz[n] is None):   # per-read artefacts (main.py:140-150)
                    for j, i in enumerate(idx):
                        tail = "forward" if fwd[j] else "reverse"
                        if args.plot and r["n_win"][j] > 0:
                            import matplotlib.pyplot as plt
                            y = sums[win_off[i]:win_off[i + 1]] / len(pattern)
                            allsteps._plot_changepoint(ids[j], y, sliding_val, args.trimfirst, int(point[j]), args.rangecp or int(m[j]))
                            plt.savefig(f"{args.outputDir}/plot_{telo_phrase}_{image_num[n] + j}.png", format="png", dpi=300)
                            plt.close()
                        if args.rawcountpattern and raw_npz[n] is None:
                            _write_rawcount(args, telo_phrase, image_num[n] + j, pattern, sliding_val, raw[win_off[i]:win_off[i + 1]], tail)
                image_num[n] += len(idx)
        ok = True
    finally:
        for _ in wthreads:
            wq.put(None)
        for t in wthreads:
            t.join()
        if out_handle is not None:
            out_handle.close()
        if not ok or werr:                                  # no half-written archive is left behind, whatever went wrong
            for w in raw_npz:
                if w is not None:
                    w.discard()
    if werr:
        raise werr[0]
    for w in raw_npz:
        if w is not None:
            w.finish()
    if out_handle is not None:
        tprint(f"Temporary fasta file with TRC more than {min_cutoff}:", fasta_temp)
        if wstat["write_s"] > 0.05:                 # (big outputs only: what bounds a run that rewrites most of its input)
            nbytes = os.path.getsize(fasta_temp)
            tprint(f"{base_name}: {wstat['records']} passing records, {nbytes} bytes written in {wstat['write_s']:.2f} thread-seconds on {len(wthreads)} writer threads "
                   f"({nbytes / wstat['write_s'] / 1e9:.2f} GB/s per thread); the scan loop waited {wstat['blocked_s']:.2f} s for them")
    st = pool.stats
    if st.get("shards", 0) > 1:
        tprint(f"{base_name}: read as {st['shards']} byte ranges, one reader team each")
    if st["heads_batches"]:
        tprint(f"{base_name}: {st['heads_batches']} of {st['batches']} batches scanned in two passes (read ends first, then the reads that pass): "
               f"{st['upload_bytes']} bytes uploaded for {st['input_bases']} bases")
    return rows


def _write_rawcount(args, telo_phrase, image_num, pattern, slide, block, tail):
    """rawcount_{k}_{i}.csv in the layout DataFrame.to_csv gives upstream (main.py:146-150)."""
    import pandas as pd
    n_win = block.shape[0]
    df = pd.DataFrame({
        "tail": tail,
        "position": np.repeat(np.arange(n_win, dtype=np.int64) * slide, len(pattern)),
        "pattern": np.tile(np.array(pattern, dtype=object), n_win),
        "count": block.reshape(-1).astype(np.int64),
    })
    df.to_csv(f"{args.outputDir}/rawcount_{telo_phrase}_{image_num}.csv")


def analysis_run(args, engines=None, engine_factory=None, wait_plots=True):
    """`engines`: contexts to use (tests inject theirs).  `engine_factory()` -> a fresh list of contexts: given (or by
    default on real GPUs), several input files are processed concurrently, one host thread + one set of contexts per
    file in flight -- the role of upstream's `Pool(num_cores)` over files (main.py:232-235)."""
    LAST_TIMINGS.clear()
    print("---- Topsicle run parameters ---")
    for k, v in vars(args).items():
        tprint(f"{k}: {v}")
    print("---------------------")
    tprint("Starting Topsicle analysis")
    # (before any file is read or written; the root of a motif that --pattern auto has yet to find is checked below)
    _check_flags(args, EARLY_CHECKS, "ACGT" if args.pattern.strip().lower() == "auto" else variants.primitive_root(args.pattern.upper()))
    if args.pattern.strip().lower() == "auto":
        # the motif comes from the reads (motif.py); from here on the run is the one `--pattern <that motif>` would have been
        if engines is None:
            engines, engine_factory = _open_engines(args, engine_factory)
        args.pattern = find_pattern(args, engines)
    if len(args.pattern) > hiplib.WIDE_MAX_K:
        # (before any file is read or written: k-mers of up to 32 letters and 64 patterns per table is what the scan kernels hold)
        tprint(f"--pattern has {len(args.pattern)} letters: motifs of up to {hiplib.WIDE_MAX_K} letters are supported")
        sys.exit(2)
    os.makedirs(args.outputDir, exist_ok=True)

    if args.threads is not None:
        num_cores = args.threads
        tprint(f"Specified number of cores are/is: {num_cores}")
    else:
        num_cores = len(os.sched_getaffinity(0))
        tprint(f"By default, Topsicle allocates nmber of cores: {num_cores}")

    output_csv = f"{args.outputDir}/telolengths_all.csv"
    tprint(f"Output will be here: {output_csv}")
    if os.path.exists(output_csv) and os.path.getsize(output_csv) > 0:
        if args.override:
            tprint(f"Output file {output_csv} already exists and will be overridden becuz having --override flag.")
            os.remove(output_csv)
        else:
            tprint(f"Output file {output_csv} already exists and is not empty. Exiting to avoid overwrite. Use --override to force overwrite.")
            sys.exit(1)

    if args.telophrase is None:
        telo_phrases = [len(args.pattern) - 2]
        tprint(f"No telophrase provided, use kmer: {telo_phrases}")
    else:
        telo_phrases = args.telophrase if isinstance(args.telophrase, list) else [args.telophrase]
    print("---------------------")

    with open(output_csv, mode="w", newline="") as fh:
        csv.writer(fh).writerow(["file_number", "phrase", "trc", "readID", "telo_length"])

    if engines is None:
        engines, engine_factory = _open_engines(args, engine_factory)

    phrase_to_telo = defaultdict(list)
    phrase_to_trc = defaultdict(list)
    phrases = []
    for telo_phrase in telo_phrases:
        if telo_phrase > len(args.pattern):
            tprint("Cannot have length of subset larger than length of pattern")
            tprint(f"Cannot get {telo_phrase}-bp cut from {len(args.pattern)}-bp pattern")
            sys.exit()
        sliding_val = args.slide if args.slide else len(args.pattern)
        pattern = allsteps.patterns_to_search(telopattern=args.pattern, cut_length=telo_phrase)
        tprint("patterns to search:", pattern)
        phrases.append((telo_phrase, pattern, sliding_val))

    # one collector per analysis and k (tracts: one for the run) for the whole run; process_file_multi hangs them on its jobs
    unit = variants.primitive_root(args.pattern.upper())
    args.analysis_collectors, args.tract_collector = [{} for _ in phrases], None
    for mod in ANALYSES:
        if not getattr(args, mod.FLAG, None):
            continue
        _check_flags(args, (mod,), unit)
        if mod.POWER_NOTE and unit != args.pattern.upper():
            tprint(f"--{mod.FLAG}: {args.pattern} is a power of {unit}; " + mod.POWER_NOTE.format(unit=unit))
        if mod is tracts:
            # the map needs whole reads on the device: no heads-only batches
            if getattr(args, "twopass", None) == "on":
                tprint("--tracts maps whole reads: --twopass on ignored")
            tprint("--tracts: every file is scanned as whole reads (--twopass off)")
            args.twopass = "off"
            args.tract_collector = tracts.cli_collector(args, unit)
            continue
        for mine, (_k, _pattern, slide) in zip(args.analysis_collectors, phrases):
            mine[mod.FLAG] = mod.cli_collector(args, unit, slide)
        if mod is ends and getattr(args, "endref", None):
            _scan_endref(args, unit, phrases, engines[0])

    filenames = []
    if os.path.isdir(args.inputDir):
        for root, _dirs, files in os.walk(args.inputDir):
            for filename in files:
                filenames.append(os.path.join(root, filename))
    else:
        filenames.append(args.inputDir)

    # every k in ONE pass over the input (the reference loops over k outermost and re-parses every file per k,
    # main.py:206-235): per file a list of row lists, one per k
    tprint("begin processing reads")
    t_reads = time.perf_counter()
    per_file = _process_files(args, filenames, phrases, engines, engine_factory, num_cores)
    LAST_TIMINGS["reads_s"] = time.perf_counter() - t_reads
    tprint("finished processing all reads")
    print("---------------------")
    for n, (telo_phrase, _pattern, _slide) in enumerate(phrases):
        late = []
        for file_rows in per_file:
            for entry in file_rows[n]:
                phrase_to_telo[entry[1]].append(float(entry[2][0][1]))
                phrase_to_trc[entry[1]].append(float(entry[3]))
                if n > 0:
                    late.append([entry[0], entry[1], "%.3f" % entry[3], entry[2][0][0], entry[2][0][1]])
        if late:                                   # rows of the later k's follow the first k's, in upstream's order
            with _CSV_LOCK, open(output_csv, mode="a", newline="") as fh:
                csv.writer(fh).writerows(late)

    for mod in PER_K_ANALYSES:
        for (telo_phrase, _pattern, _slide), mine in zip(phrases, args.analysis_collectors):
            if mod.FLAG in mine:
                for line in mod.finish_and_write(args, telo_phrase, mine[mod.FLAG], filenames, engines):
                    tprint(line)
    if args.tract_collector is not None:
        for line in tracts.finish_and_write(args, None, args.tract_collector, filenames, engines):
            tprint(line)

    t_sum = time.perf_counter()
    summarize(args, phrase_to_telo, phrase_to_trc)
    LAST_TIMINGS["summary_s"] = time.perf_counter() - t_sum
    tprint("All telomere found, have a nice day.")
    if wait_plots:
        wait_for_plots()


def _check_flags(args, mods, root):
    """The flags of the analyses that are switched on against `root`, the motif's primitive root: the run ends with one message at
    the first that does not hold."""
    for mod in mods:
        why = mod.cli_check(args, root) if getattr(args, mod.FLAG, None) else None
        if why is not None:
            tprint(f"--{mod.FLAG} needs {why}")
            sys.exit(2)


def _scan_endref(args, unit, phrases, engine):
    """--endref: the reference's ends -- its pieces scanned like reads, every k's table at once, into end collectors of their own that
    keep the windows -- left with the run's end collectors (ends.finish_and_write names the reads against them)."""
    own = [ends.cli_collector(args, unit, slide, anchor=True) for _k, _pattern, slide in phrases]
    ref_ends = endref.scan_reference(args.endref, engine, [batch.Job(pattern, _scan_params(args, slide), ends=col.spec)
                                                           for (_k, pattern, slide), col in zip(phrases, own)],
                                     own, args.maxlengthtelo, args.endminkmers)
    for (telo_phrase, _pattern, _slide), listed, mine in zip(phrases, ref_ends, args.analysis_collectors):
        if sum(e.indexed for e in listed) > endref.MAX_REFS:
            tprint(f"--endref: {sum(e.indexed for e in listed)} usable reference ends for k = {telo_phrase}, {endref.MAX_REFS} at most")
            sys.exit(2)
        mine["ends"].ref_ends = listed


def _open_engines(args, engine_factory):
    """(contexts, the factory that made them): by default two contexts per GPU of --gpus, from --device on."""
    n_gpus = max(1, getattr(args, "gpus", 1) or 1)
    first = getattr(args, "device", 0) or 0
    if engine_factory is None:
        def engine_factory():
            # two contexts (launch queues) per GPU: the upload / launch ramp / download of one batch overlaps the scan of another
            return [hiplib.HipScanner(first + i // CONTEXTS_PER_GPU) for i in range(n_gpus * CONTEXTS_PER_GPU)]
    engines = engine_factory()
    tprint(f"GPU engines: {[e.device_info() for e in engines]}")
    return engines, engine_factory


def find_pattern(args, engines):
    """`--pattern auto`: the motif census of the input's read ends (motif.find_motif, the reads --minSeqLength lets through), its
    table in the log, and the rank-1 motif -- or the end of the run, with the candidates, when too few read ends agree on one."""
    tprint("--pattern auto: looking for the repeat at the read ends")
    rows, n_reads = motif.find_motif(args.inputDir, engines, min_len=args.minSeqLength, max_reads=getattr(args, "motifreads", motif.MOTIF_READS))
    tprint(f"motif census of {n_reads} reads:")
    for line in motif.format_table(rows):
        tprint(line)
    why = motif.verdict(rows)
    if why:
        tprint(f"--pattern auto found no motif: {why}. Candidates: {[r[0] for r in rows[:10]]}. Give the motif with --pattern.")
        sys.exit(2)
    tprint(f"--pattern auto: using {rows[0][0]} ({rows[0][2]} of {sum(r[2] for r in rows)} voting read ends)")
    return rows[0][0]


def _process_files(args, filenames, phrases, engines, engine_factory, num_cores):
    """All input files: sequentially on the given contexts, or -- several files, a factory for more contexts, no per-read
    plots (pyplot is not thread-safe) -- up to min(num_cores, 8) files at a time, each on its own thread and contexts
    (parsing / gunzip is the bottleneck, the GPUs are shared).  Results keep file order: one list of per-k row lists per file."""
    workers = min(len(filenames), max(1, num_cores), 8)
    # (per-read plots and per-read CSVs go through pyplot / pandas on the calling thread; the npz archive is written natively by
    # the batch workers, one archive per file: nothing is shared between files)
    per_read_files = args.plot or (args.rawcountpattern and getattr(args, "rawcountformat", "csv") != "npz")
    if workers <= 1 or engine_factory is None or per_read_files:
        return [process_file_multi(args, seq_loc, phrases, engines) for seq_loc in filenames]
    import threading
    from concurrent.futures import ThreadPoolExecutor
    local = threading.local()
    made = []

    def work(seq_loc):
        if not hasattr(local, "engines"):
            local.engines = engine_factory()
            made.append(local.engines)
        return process_file_multi(args, seq_loc, phrases, local.engines)

    tprint(f"processing {len(filenames)} files, {workers} at a time")
    try:
        with ThreadPoolExecutor(max_workers=workers) as ex:
            return list(ex.map(work, filenames))
    finally:
        for engs in made:
            for e in engs:
                e.close()


def recommend_cutoff(vertex_x, max_trc, median_trc, inputtrc):
    """The cutoff advice of main.py:276-293 as a pure function: (recommended cutoff, log lines).  The fit's vertex is
    accepted unless it lies beyond the data (then the median TRC, or 0.9 if that is >= 1) or is implausibly low (< 0.4:
    the input cutoff takes over when it is higher)."""
    notes = []
    if vertex_x > max_trc:
        notes.append(f"Asymptotic TRC {vertex_x:.3f} is greater than max TRC, which is not expected. See plot.")
        use_median = median_trc < 1.0
        notes.append(f"Using median TRC value ({median_trc:.3f}) as asymptotic TRC instead." if use_median
                     else "Using 0.9 as asymptotic TRC instead, since asymptotic is greater than 1.0.")
        vertex_x = median_trc if use_median else 0.9
    if vertex_x < 0.4:
        notes.append("Quadratic fit suggests asymptotic TRC less than 0.4. See plot with fit line")
        if max_trc < 0.4:
            notes.append(f"Maximum TRC value in data is {max_trc:.3f}, which is less than 0.4, indicating low confidence in telomere detection.")
        if vertex_x < inputtrc:
            notes.append(f"Asymptotic TRC {vertex_x:.3f} is less than input cutoff {inputtrc:.3f}. Topsicle declares input TRC (={inputtrc}) as asymptotic TRC.")
            vertex_x = inputtrc
    return vertex_x, notes


def summarize(args, phrase_to_telo, phrase_to_trc):
    """Per-k medians and the quadratic-fit cutoff advice (main.py:248-306)."""
    inputtrc = args.cutoff[0] if isinstance(args.cutoff, (list, tuple)) else args.cutoff
    for phrase in sorted(phrase_to_telo):
        telo = np.asarray(phrase_to_telo[phrase], dtype=np.float64)
        trc = np.asarray(phrase_to_trc[phrase], dtype=np.float64)
        tprint(f"k-mer: {phrase}, with TRC >= {inputtrc}, median telomere length is {np.median(telo):.2f} bp")
        if len(telo) < 3:
            tprint("Not enough data points to recommend TRC cutoff.")
            continue
        median_trc = np.median(trc)
        fit_x, fit_y, coeffs = allsteps.fit_quadratic_and_find_vertex(list(trc), list(telo), inputtrc=inputtrc, median_trc=median_trc)
        # the picture is drawn on a helper thread: the numbers below do not wait for it (0.2 s of a 0.4 s run on 10 000 reads)
        png = os.path.join(args.outputDir, f"quadfit_{phrase}mer_{args.pattern}.png")
        _submit_plot(allsteps.plot_quadratic_fit, (trc, telo, coeffs, fit_x, fit_y, png), png)
        cutoff, notes = recommend_cutoff(fit_x, float(trc.max()), median_trc, inputtrc)
        for line in notes:
            tprint(line)
        tprint(f"asymptotic TRC, or recommended cutoff: {cutoff:.3f}")
        kept = telo[trc >= cutoff]
        if len(kept):
            tprint(f"Median telomere length for reads with TRC cutoff >= {cutoff:.3f}: {np.median(kept):.2f} bp")
        else:
            tprint(f"No read has TRC >= {cutoff:.3f}, please double check the data or submit log to GitHub.")


def build_parser():
    parser = argparse.ArgumentParser(description="Topsicle - Telomere length estimation from long reads (MI355X build)",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("--inputDir", "-i", type=str, metavar="FILE/FOLDER", help="Required, Path to the input file or directory", required=True)
    parser.add_argument("--outputDir", "-o", type=str, metavar="FOLDER", help="Required, Path to the output directory", required=True)
    parser.add_argument("--pattern", metavar="CHAR", type=str, help="Required, Telomere repeat sequence (in 5' to 3' orientation). For e.g., in human use CCCTAA (MI355X build: 'auto' finds it from the read ends first)", required=True)
    parser.add_argument("--minSeqLength", metavar="INT", type=int, help="Minimum length of a long read sequence that will be analyzed", default=9000)
    parser.add_argument("--rawcountpattern", action="store_true", help="Output raw count of the k-mer for each window")
    parser.add_argument("--rawcountformat", choices=["csv", "npz"], default="csv",
                        help="(extension) csv: one rawcount_{k}_{i}.csv per read like upstream; npz: one columnar rawcount_{k}_{file}.npz per input file and k")
    parser.add_argument("--telophrase", nargs="+", metavar="INT", type=int, help="Length of telomere k-mer to search. By default will use telomere k-mer length minus 2")
    parser.add_argument("--cutoff", nargs="+", metavar="FLOAT", type=float, help="TRC statistics threshold", default=0.7)
    parser.add_argument("--windowSize", metavar="INT", type=int, help="Sliding window size", default=100)
    parser.add_argument("--slide", metavar="INT", type=int, help="Window sliding step. Default is telomere k-mer length")
    parser.add_argument("--trimfirst", metavar="INT", type=int, help="Length of intial number of base pairs to trim", default=100)
    parser.add_argument("--maxlengthtelo", metavar="INT", type=int, help="Longest possible length of telomere for any given read", default=20000)
    parser.add_argument("--plot", action="store_true", help="Optional, generate plot showing for each telomere read the abundance across the sequencing reead and the changepoint")
    parser.add_argument("--rangecp", metavar="INT", type=int, help="Optional, set range of changepoint plot for visualization, default is maxlengthtelo")
    parser.add_argument("--read_check", metavar="STR", type=str, help="Optional, get telomere of a specific read")
    parser.add_argument("--override", "-ov", action="store_true", help="Override telolengths_all.csv file but keep subset fastq")
    parser.add_argument("--threads", "-t", metavar="INT", type=int, help="Number of CPU cores to use (by default, all available cores)", default=None)
    # MI355X build only
    parser.add_argument("--gpus", metavar="INT", type=int, default=1, help="GPUs of this node to shard reads over")
    parser.add_argument("--device", metavar="INT", type=int, default=0, help="index of the first GPU to use")
    parser.add_argument("--shards", metavar="INT", type=int, default=0,
                        help="MI355X build: cut ONE plain input file into this many byte ranges, each decoded by a reader thread team of its own "
                             "(0 = one per GPU when the file has at least 256 MiB per GPU; compressed files keep one reader)")
    parser.add_argument("--variants", action="store_true",
                        help="MI355X build: census of the called telomere tracts -- canonical repeats, repeats with one substituted letter (by place and letter), "
                             "the rest -- per read (variants_{k}.csv) and per distance from the boundary (variant_profile_{k}.csv)")
    parser.add_argument("--variantbin", metavar="INT", type=int, default=variants.DEFAULT_BIN, help="--variants: width of a profile bin in bases (64..4064)")
    parser.add_argument("--variantbins", metavar="INT", type=int, default=variants.DEFAULT_BINS, help="--variants: bins of the profile, the last takes everything beyond (1..64)")
    parser.add_argument("--ends", action="store_true",
                        help="MI355X build: group the telomeric reads by chromosome end from a sketch of the subtelomere behind each called boundary -- one row "
                             "per read (end_reads_{k}.csv) and one per group (ends_{k}.csv); groups of reads, not chromosome names")
    parser.add_argument("--endspan", metavar="INT", type=int, default=ends.DEFAULT_SPAN, help="--ends: bases behind the boundary that are sketched (endk..16384; never beyond maxlengthtelo)")
    parser.add_argument("--endk", metavar="INT", type=int, default=ends.DEFAULT_K, help="--ends: k-mer length of the sketch (8..16)")
    parser.add_argument("--endbuckets", metavar="INT", type=int, default=ends.DEFAULT_BUCKETS, help="--ends: buckets of a sketch (64, 128, 256 or 512)")
    parser.add_argument("--endminmatch", metavar="INT", type=int, default=ends.DEFAULT_MIN_MATCH, help="--ends: equal buckets that link two reads (1..endbuckets)")
    parser.add_argument("--endminkmers", metavar="INT", type=int, default=ends.DEFAULT_MIN_KMERS, help="--ends: subtelomere k-mers a read needs to take part")
    parser.add_argument("--endminreads", metavar="INT", type=int, default=ends.DEFAULT_MIN_READS, help="--ends: reads a group needs to be reported as an end")
    parser.add_argument("--anchor", action="store_true",
                        help="MI355X build, with --ends: place the reads of every end group on their group's reference read, agree on one boundary per "
                             "group and measure every read's telomere to it (anchored_reads_{k}.csv, anchored_ends_{k}.csv); needs --endspan of at most 4096")
    parser.add_argument("--anchorminvotes", metavar="INT", type=int, default=anchor.DEFAULT_MIN_VOTES, help="--anchor: k-mer votes a read needs on its best diagonals to be anchored")
    parser.add_argument("--anchorratio", metavar="INT", type=int, default=anchor.DEFAULT_RATIO, help="--anchor: ... and how many times the votes of the runner-up diagonals")
    parser.add_argument("--consensus", action="store_true",
                        help="MI355X build, with --ends --anchor: align the anchored reads of every end group base by base and call one consensus subtelomere per "
                             "group (end_consensus_{k}.fa and .csv, consensus_reads_{k}.csv) and a reference --endref takes in the next run (end_reference_{k}.fa)")
    parser.add_argument("--consensusmindepth", metavar="INT", type=int, default=consensus.DEFAULT_MIN_DEPTH, help="--consensus: reads a column needs to be called from them")
    parser.add_argument("--endref", metavar="REF", default=None,
                        help="MI355X build, with --ends: name the end groups against a reference -- a FASTA or FASTQ (plain or gzip) of chromosomes, contigs or subtelomeres; the "
                             "first and last maxlengthtelo bases of every record are scanned like reads, and every read's window is placed on the ends found "
                             "(ref_ends_{k}.csv, named_reads_{k}.csv, named_ends_{k}.csv); needs --endspan of at most 4096")
    parser.add_argument("--endrefmaxocc", metavar="INT", type=int, default=endref.DEFAULT_MAX_OCC, help="--endref: a k-mer that occurs more often than this over all reference ends takes no part (1..64)")
    parser.add_argument("--endrefminvotes", metavar="INT", type=int, default=endref.DEFAULT_MIN_VOTES, help="--endref: k-mer votes a read needs on its best diagonals to be named")
    parser.add_argument("--endrefratio", metavar="INT", type=int, default=endref.DEFAULT_RATIO, help="--endref: ... and how many times the votes of the runner-up diagonals")
    parser.add_argument("--adapters", metavar="FILE|SEQ", nargs="+", default=None,
                        help="MI355X build: locate adapters at the telomere end of every read with a called boundary -- a FASTA / FASTQ of named sequences, or "
                             "literal sequences (adapter1 ...), 12..64 letters of ACGT each, 64 at most, given as they stand in front of the --pattern repeats; one row "
                             "per read (adapters_{k}.csv: adapter, edit distance, where it ends, the length measured from there) and one per sequence "
                             "(adapter_summary_{k}.csv)")
    parser.add_argument("--refine", action="store_true",
                        help="MI355X build: the boundary of every read with a called one again at base resolution, with what supports it -- one change point on "
                             "the per-position hits of the --pattern repeat over [trimfirst, maxlengthtelo); one row per read (refined_{k}.csv: refined length, "
                             "shift against telo_length, score, drop, margin, the called boundary's deficit, hit densities, class) and one per class "
                             "(refine_summary_{k}.csv); no other output changes")
    parser.add_argument("--refinehit", metavar="INT", type=int, default=refine.DEFAULT_HIT, help="--refine: what a position whose word is within one substitution of the repeat adds (1..16)")
    parser.add_argument("--refinemiss", metavar="INT", type=int, default=refine.DEFAULT_MISS, help="--refine: what any other position costs (1..16)")
    parser.add_argument("--refinesep", metavar="INT", type=int, default=refine.DEFAULT_SEP, help="--refine: positions the runner-up boundary must be away from the best (1..65535)")
    parser.add_argument("--refineminscore", metavar="INT", type=int, default=refine.DEFAULT_MIN_SCORE, help="--refine: a read whose best score is below this is classed no_telomere")
    parser.add_argument("--refinemindrop", metavar="INT", type=int, default=refine.DEFAULT_MIN_DROP, help="--refine: a read whose score falls by less than this up to the end of the region is classed open")
    parser.add_argument("--refineminmargin", metavar="INT", type=int, default=refine.DEFAULT_MIN_MARGIN, help="--refine: a read whose runner-up boundary scores within this of the best is classed ambiguous")
    parser.add_argument("--methyl", action="store_true",
                        help="MI355X build, BAM input: CpG methylation of the subtelomere behind every called boundary from the records' MM / ML tags -- one row per "
                             "read (methyl_{k}.csv: tag status, CpGs, calls, high and low calls, meth_fraction, mean probability), one per bin of distance "
                             "from the boundary (methyl_profile_{k}.csv) and, with --ends, one per end group (methyl_ends_{k}.csv); no other output changes")
    parser.add_argument("--methylbin", metavar="INT", type=int, default=methyl.DEFAULT_BIN, help="--methyl: width of a bin in bases (16..4096)")
    parser.add_argument("--methylbins", metavar="INT", type=int, default=methyl.DEFAULT_BINS, help="--methyl: bins behind the boundary, in the subtelomere")
    parser.add_argument("--methyltract", metavar="INT", type=int, default=methyl.DEFAULT_TRACT, help="--methyl: bins in front of the boundary, in the tract (64 bins and 16384 bases at most together)")
    parser.add_argument("--methylhigh", metavar="FLOAT", type=float, default=methyl.DEFAULT_HIGH, help="--methyl: a call with at least this probability counts as methylated")
    parser.add_argument("--methyllow", metavar="FLOAT", type=float, default=methyl.DEFAULT_LOW, help="--methyl: a call with at most this probability counts as unmethylated")
    parser.add_argument("--methylcode", metavar="CHAR", type=str, default=methyl.DEFAULT_CODE, help="--methyl: the modification code of the MM tag (m: 5mC, h: 5hmC)")
    parser.add_argument("--adaptersearch", metavar="INT", type=int, default=adapters.DEFAULT_SEARCH, help="--adapters: bases at the telomere end that are searched (16..1024; never beyond maxlengthtelo)")
    parser.add_argument("--adaptererr", metavar="FLOAT", type=float, default=adapters.DEFAULT_ERR, help="--adapters: edits allowed per letter of a sequence (a sequence of m letters: floor(err m) edits)")
    parser.add_argument("--adaptermargin", metavar="INT", type=int, default=adapters.DEFAULT_MARGIN, help="--adapters: edits by which the best sequence must beat every other to name the read")
    parser.add_argument("--tracts", action="store_true",
                        help="MI355X build: map the telomere-repeat tracts of every WHOLE read, on both strands -- one row per tract (tracts.csv) and one per "
                             "read with a tract and its class: fusion, both_ends, interstitial, terminal (tract_reads.csv).  Runs the files as --twopass off")
    parser.add_argument("--tractblock", metavar="INT", type=int, default=tracts.DEFAULT_BLOCK, help="--tracts: positions per block (a multiple of 64 in 64..1024)")
    parser.add_argument("--tractminhits", metavar="INT", type=int, default=tracts.DEFAULT_MIN_HITS, help="--tracts: hits that flag a block (1..tractblock)")
    parser.add_argument("--tractgap", metavar="INT", type=int, default=tracts.DEFAULT_GAP, help="--tracts: unflagged blocks a tract may bridge (0..64)")
    parser.add_argument("--tractminblocks", metavar="INT", type=int, default=tracts.DEFAULT_MIN_BLOCKS, help="--tracts: blocks a tract spans at least (1..64)")
    parser.add_argument("--tractedge", metavar="INT", type=int, default=tracts.DEFAULT_EDGE,
                        help="--tracts: a tract within this many bases of the read's end counts as terminal; the widest gap between the two tracts of a fusion")
    parser.add_argument("--twopass", choices=["auto", "on", "off"], default=None,
                        help="MI355X build: upload only the two 1000-base ends of every read for the TRC filter and the scanned part of the "
                             "reads that pass afterwards (auto, the default unless $TOPSICLE_TWO_PASS says otherwise: while few reads of a batch pass, "
                             "as in whole-genome read sets)")
    return parser


def main(argv=None):
    start_time = time.time()
    args = build_parser().parse_args(argv)
    tprint.logfile = get_log_path(args)
    warm_up_plotting()
    analysis_run(args, wait_plots=False)
    # the elapsed time is that of the ANALYSIS: the summary PNGs may still be rendering on the plot thread -- the process waits
    # for them when it ends (atexit), a caller of main() can call wait_for_plots() itself
    print(f"Elapsed time(s): {time.time() - start_time:.2f} seconds")


if __name__ == "__main__":
    main()
