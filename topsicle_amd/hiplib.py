"""ctypes binding of libtopsicle_hip.so (C ABI: include/topsicle_hip.h).

This is the only way the package reaches the GPU.  There is deliberately NO CPU fallback:
if the shared library is missing, cannot be loaded, or no MI355X is visible, every entry
point raises `TopsicleHipError` -- results never silently come from anywhere else.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

LIB_NAME = "libtopsicle_hip.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

# flags (TPS_F_*)
F_STEP1, F_WINDOWS, F_BINSEG, F_STORE_SUMS, F_STORE_RAW, F_TAILS_IN = 1, 2, 4, 8, 16, 32
MAX_K, MAX_PATTERNS, MAX_SLOTS = 15, 31, 16
WIDE_MAX_K, WIDE_MAX_PATTERNS = 32, 64      # tps_set_patterns_wide (TPS_WIDE_MAX_K, TPS_WIDE_MAX_PATTERNS)
FOLLOW_MAX_FWD, FOLLOW_WIDE_MAX_FWD, FOLLOW_HIST_MAX = 15, 32, 8      # k-mers tps_batch_kmer_followers / _wide take; most following letters with a histogram

EXPORTS = [
    "tps_abi_version", "tps_device_count", "tps_ctx_create", "tps_ctx_destroy", "tps_last_error",
    "tps_set_patterns", "tps_set_patterns_wide", "tps_batch_upload", "tps_batch_upload_packed", "tps_batch_upload_nib4", "tps_batch_share", "tps_host_alloc", "tps_host_free",
    "tps_batch_download_packed", "tps_batch_kmer_followers", "tps_batch_kmer_followers_wide", "tps_batch_motif_census", "tps_batch_variant_census", "tps_batch_tract_map", "tps_batch_end_sketch", "tps_sketch_links", "tps_batch_end_window", "tps_window_offsets", "tps_window_place", "tps_window_align", "tps_batch_adapter_find", "tps_batch_boundary_refine", "tps_batch_mod_profile", "tps_batch_set_tails", "tps_batch_scan", "tps_sync",
    "tps_batch_results", "tps_batch_window_offsets", "tps_batch_window_sums", "tps_batch_window_raw",
    "tps_batch_raw_to_fd", "tps_batch_trc_counts", "tps_trc_counts", "tps_window_counts", "tps_binseg_l2", "tps_binseg_l2_ties", "tps_batch_read_sums", "tps_window_count",
    "tps_kernel_time_ms", "tps_kernel_time_reset", "tps_device_info", "tps_batch_kernel_info", "tps_ctx_debug_option", "tps_debug_stamps_get",
]


class TopsicleHipError(RuntimeError):
    pass


class Params(C.Structure):
    """struct tps_params -- names follow the reference CLI (Topsicle/main.py:319-334)."""
    _fields_ = [("no_bp", C.c_int32), ("min_len", C.c_int32), ("min_count", C.c_int32),
                ("window", C.c_int32), ("slide", C.c_int32), ("trimfirst", C.c_int32),
                ("maxlen", C.c_int32), ("jump", C.c_int32), ("min_size", C.c_int32),
                ("flags", C.c_uint32)]


DESC_DTYPE = np.dtype([("word_off", "<i8"), ("len", "<i4"), ("flags", "<u4")], align=True)      # struct tps_read_desc
assert DESC_DTYPE.itemsize == 16
RD_HAS_INVALID = 1

NIB_SRC_DTYPE = np.dtype([("off", "<i8"), ("flags", "<u4"), ("reserved", "<u4")], align=True)    # struct tps_nib_src
assert NIB_SRC_DTYPE.itemsize == 16
NIB_REVERSE = 1        # TPS_NIB_REVERSE: a reverse-strand BAM record (the read is the reverse complement of its stored codes)

RESULT_DTYPE = np.dtype([("best_start", "<i4"), ("best_start_idx", "<i4"), ("best_end", "<i4"),
                         ("best_end_idx", "<i4"), ("tail", "<i4"), ("pass", "<i4"), ("n_win", "<i4"),
                         ("bkp", "<i4"), ("gain", "<f8"), ("flags", "<u4"), ("reserved", "<u4")], align=True)
assert RESULT_DTYPE.itemsize == 48
MOTIF_HIT_DTYPE = np.dtype([("unit", "<u8"), ("period", "<i4"), ("support", "<i4"), ("run_start", "<i4"), ("run_len", "<i4"),
                            ("n_bases", "<i4"), ("reserved", "<i4")], align=True)                          # struct tps_motif_hit
assert MOTIF_HIT_DTYPE.itemsize == 32
MOTIF_MAX_PERIOD, MOTIF_MAX_SPAN = 32, 4096      # tps_batch_motif_census: the longest period, the most bases of a read end
VARIANT_MAX_UNIT, VARIANT_BIN_RANGE, VARIANT_MAX_BINS = 32, (64, 4064), 64      # tps_batch_variant_census: letters of the unit, bin width, bins
TRACT_DTYPE = np.dtype([("begin", "<i4"), ("end", "<i4"), ("hits", "<i4"), ("blocks", "<i4")])             # struct tps_tract
assert TRACT_DTYPE.itemsize == 16
# tps_batch_tract_map: letters of the unit, block (a multiple of 64), gap, min_blocks, max_tracts; min_hits is 1..block
TRACT_UNIT_RANGE, TRACT_BLOCK_RANGE, TRACT_GAP_RANGE, TRACT_MIN_BLOCKS_RANGE, TRACT_MAX_TRACTS_RANGE = (4, 32), (64, 1024), (0, 64), (1, 64), (1, 16)
# tps_batch_end_sketch: k, buckets, end - begin; tps_sketch_links: sketches, links kept per row
ENDS_K_RANGE, ENDS_BUCKETS, ENDS_MAX_WINDOW, LINKS_MAX_N, LINKS_MAX_LINKS = (8, 16), (64, 128, 256, 512), 16384, 262144, 256
ENDS_EMPTY = 0xFFFFFFFF           # an empty bucket of a sketch
# tps_batch_end_window / tps_window_offsets: letters of a window, rows of one call
ANCHOR_MAX_SPAN, ANCHOR_MAX_ROWS = 4096, 262144
# tps_window_place: reference rows of one call, entries of a k-mer that still takes part
PLACE_MAX_REFS, PLACE_MAX_OCC = 1024, 64
# tps_window_align: letters of a window, rows of either set, entries of a stat row and of a pile column; the two flags; a column's states
ALIGN_MAX_SPAN, ALIGN_MAX_ROWS, ALIGN_STATS, ALIGN_PILE = 4096, 262144, 6, 13
ALIGN_NONE, ALIGN_EDGE, ALIGN_DELETED, ALIGN_UNCOVERED = 1, 2, 4, 7
# tps_batch_adapter_find: letters of a pattern, patterns of one call, letters of a region
ADAPTER_LEN_RANGE, ADAPTER_MAX_PATTERNS, ADAPTER_MAX_REGION = (12, 64), 64, 1024
REFINE_DTYPE = np.dtype([(f, "<i4") for f in ("pos", "score", "drop", "at_score", "hits_before", "hits_after", "runner", "runner_pos")])      # struct tps_refine
assert REFINE_DTYPE.itemsize == 32
# tps_batch_boundary_refine: hit and miss, sep, end - begin (after end is clamped to the read)
REFINE_WEIGHT_RANGE, REFINE_SEP_RANGE, REFINE_MAX_REGION = (1, 16), (1, 65535), 65536
MOD_ROW_DTYPE = np.dtype([(f, "<u4") for f in ("c_total", "entries", "beyond", "in_region", "off_context", "cpg", "called", "flags")])      # struct tps_mod_row
MOD_BIN_DTYPE = np.dtype([("cpg", "<u2"), ("called", "<u2"), ("high", "<u2"), ("low", "<u2"), ("sum", "<u4")])                                    # struct tps_mod_bin
assert MOD_ROW_DTYPE.itemsize == 32 and MOD_BIN_DTYPE.itemsize == 12
# tps_batch_mod_profile: the bin width, the bins, end - begin (after end is clamped to the read); tps_mod_row.flags
MOD_W_RANGE, MOD_MAX_BINS, MOD_MAX_REGION, MOD_BAD = (16, 4096), 64, 16384, 1
RES_TIE = 1            # TPS_RES_TIE: the exact tournament decided the change-point (candidates within float64 noise of each other)


def make_params(no_bp=1000, min_len=0, min_count=-1, window=100, slide=6, trimfirst=100, maxlen=20000,
                jump=5, min_size=2, flags=F_STEP1 | F_WINDOWS | F_BINSEG) -> Params:
    return Params(no_bp, min_len, min_count, window, slide, trimfirst, maxlen, jump, min_size, flags)


_lib = None


def load_library(path: str | None = None) -> C.CDLL:
    """Load libtopsicle_hip.so (built in-tree by `__graft_entry__.build()` / `make`)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("TOPSICLE_HIP_LIB") or LIB_PATH      # TOPSICLE_HIP_LIB: e.g. the diagnostics build with phase stamps
    if not os.path.exists(p):
        raise TopsicleHipError(f"{p} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()'). "
                               "topsicle_amd has no CPU fallback.")
    try:
        lib = C.CDLL(p)
    except OSError as e:
        raise TopsicleHipError(f"cannot load {p}: {e}") from e
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    proto = {
        "tps_abi_version": (C.c_int, []),
        "tps_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "tps_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "tps_ctx_destroy": (C.c_int, [vp]),
        "tps_last_error": (C.c_char_p, []),
        "tps_set_patterns": (C.c_int, [vp, C.c_char_p, i32, i32]),
        "tps_set_patterns_wide": (C.c_int, [vp, C.c_char_p, i32, i32]),
        "tps_batch_upload": (C.c_int, [vp, i32, vp, vp, i64]),
        "tps_batch_upload_packed": (C.c_int, [vp, i32, vp, vp, vp, i64, i64]),
        "tps_batch_upload_nib4": (C.c_int, [vp, i32, vp, i64, vp, vp, i64, i64]),
        "tps_batch_share": (C.c_int, [vp, i32, vp, i32]),
        "tps_host_alloc": (C.c_int, [vp, i64, C.POINTER(vp)]),
        "tps_host_free": (C.c_int, [vp, vp]),
        "tps_batch_download_packed": (C.c_int, [vp, i32, vp, vp, vp, i64, i64, C.POINTER(i64)]),
        "tps_batch_kmer_followers": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, vp, i64, vp, i64]),
        "tps_batch_kmer_followers_wide": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, vp, i64, vp, i64]),
        "tps_batch_motif_census": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, vp, i64, vp, i64]),
        "tps_batch_variant_census": (C.c_int, [vp, i32, C.c_uint64, i32, vp, vp, vp, i64, i32, i32, vp, i64, vp, i64]),
        "tps_batch_tract_map": (C.c_int, [vp, i32, C.c_uint64, i32, i32, i32, i32, i32, i32, vp, i64, vp, i64, vp, i64]),
        "tps_batch_end_sketch": (C.c_int, [vp, i32, C.c_uint64, i32, i32, i32, vp, vp, vp, i64, vp, i64, vp, i64]),
        "tps_sketch_links": (C.c_int, [vp, vp, i64, i32, i64, i32, i32, vp, i64, vp, i64, vp, i64]),
        "tps_batch_end_window": (C.c_int, [vp, i32, C.c_uint64, i32, i32, vp, vp, vp, i64, i32, vp, i64, vp, i64]),
        "tps_window_offsets": (C.c_int, [vp, vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, i64]),
        "tps_window_place": (C.c_int, [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64]),
        "tps_window_align": (C.c_int, [vp, vp, i64, vp, i64, vp, i64, vp, i32, vp, vp, i32, vp, i64, vp, i64, vp, vp, i32, i64]),
        "tps_batch_adapter_find": (C.c_int, [vp, i32, vp, vp, i32, vp, vp, vp, i64, vp, i64]),
        "tps_batch_boundary_refine": (C.c_int, [vp, i32, C.c_uint64, i32, vp, vp, vp, vp, i64, i32, i32, i32, vp, i64]),
        "tps_batch_mod_profile": (C.c_int, [vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, i64, i32, i32, i32, i32, i32, vp, i64, vp, i64]),
        "tps_batch_set_tails": (C.c_int, [vp, i32, vp]),
        "tps_batch_scan": (C.c_int, [vp, i32, C.POINTER(Params)]),
        "tps_sync": (C.c_int, [vp]),
        "tps_batch_results": (C.c_int, [vp, i32, vp, i64]),
        "tps_batch_window_offsets": (C.c_int, [vp, i32, vp, i64]),
        "tps_batch_window_sums": (C.c_int, [vp, i32, vp, i64]),
        "tps_batch_window_raw": (C.c_int, [vp, i32, vp, i64]),
        "tps_batch_raw_to_fd": (C.c_int, [vp, i32, vp, i64, C.c_int, i64, vp, C.POINTER(C.c_uint32), C.POINTER(i64)]),
        "tps_batch_trc_counts": (C.c_int, [vp, i32, vp, vp, i64]),
        "tps_trc_counts": (C.c_int, [vp, vp, vp, i64, i32, vp, vp]),
        "tps_window_counts": (C.c_int, [vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, vp]),
        "tps_binseg_l2": (C.c_int, [vp, vp, vp, i64, i32, i32, i32, vp, vp]),
        "tps_binseg_l2_ties": (C.c_int, [vp, vp, vp, i64, i32, i32, i32, vp, vp, vp]),
        "tps_batch_read_sums": (C.c_int, [vp, i32, i64, vp, i64]),
        "tps_window_count": (i64, [i64, i32, i32, i32, i32]),
        "tps_kernel_time_ms": (C.c_int, [vp, C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "tps_kernel_time_reset": (C.c_int, [vp]),
        "tps_device_info": (C.c_int, [vp, C.c_char_p, i32]),
        "tps_batch_kernel_info": (C.c_int, [vp, i32, C.c_char_p, i32]),
        "tps_ctx_debug_option": (C.c_int, [vp, C.c_char_p, i64]),
        "tps_debug_stamps_get": (C.c_int, [vp, i32, vp, i64]),
    }
    for name, (res, args) in proto.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise TopsicleHipError(f"{p} does not export {name}") from e
        fn.restype, fn.argtypes = res, args
    if path is None:
        _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def needs_wide(patterns) -> bool:
    """The table is beyond what set_patterns takes (k > MAX_K letters or more than MAX_PATTERNS patterns): it goes through
    set_patterns_wide and the wide kernel.  Every other table keeps the narrow call."""
    return bool(patterns) and (len(patterns[0]) > MAX_K or len(patterns) > MAX_PATTERNS)


def set_table(engine, patterns):
    """set_patterns for a narrow table, set_patterns_wide for one that needs it: what every scan site of the package calls."""
    if needs_wide(patterns):
        engine.set_patterns_wide(patterns)
    else:
        engine.set_patterns(patterns)


def debug_options_from_env() -> dict:
    """$TOPSICLE_HIP_DEBUG = "key=value,key" -> {key: int}: the one environment variable through which diagnostics reach the
    library (tps_ctx_debug_option; the library itself reads no environment).  Unset in normal use."""
    out = {}
    for item in os.environ.get("TOPSICLE_HIP_DEBUG", "").split(","):
        item = item.strip()
        if item:
            key, _, val = item.partition("=")
            out[key.strip()] = int(val) if val.strip() else 1
    return out


_crc_cb = None


def _crc32_callback():
    """Address of libtopsicle_io.so's tps_crc32 (the checksum tps_batch_raw_to_fd runs over what it writes)."""
    global _crc_cb
    if _crc_cb is None:
        from . import seqio
        lib = seqio._load_io()
        if lib is None:
            raise TopsicleHipError("libtopsicle_io.so is not built (its tps_crc32 checksums the raw-count archive)")
        _crc_cb = C.cast(lib.tps_crc32, C.c_void_p)
    return _crc_cb


def pack_reads(seqs) -> tuple[np.ndarray, np.ndarray]:
    """Concatenate read strings/bytes into (bases u8, offsets i64[n+1])."""
    bs = [s.encode("ascii", "replace") if isinstance(s, str) else bytes(s) for s in seqs]
    offsets = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=offsets[1:])
    bases = np.frombuffer(b"".join(bs), dtype=np.uint8) if bs else np.zeros(0, np.uint8)
    return np.ascontiguousarray(bases), offsets


def window_count(read_len: int, window: int, slide: int, trimfirst: int, maxlen: int) -> int:
    """Windows seq_cut_windows yields for one read (allsteps.py:219, 263-271)."""
    ns = min(read_len, maxlen) - trimfirst
    if window < 1 or slide < 1 or ns < window:
        return 0
    return (ns - window) // slide + 1


def binseg_l2_float64(y, jump: int = 5, min_size: int = 2):
    """`rpt.Binseg(model="l2").fit(y).predict(n_bkps=1)` in ruptures' own float64 arithmetic (allsteps.py:310-311; ruptures
    1.1.9: CostL2.error = signal[a:b].var(axis=0).sum() * (b - a), candidates range(0, n, jump) with both sides >= min_size,
    max() over (gain, bkp) tuples).  HOST arithmetic on purpose, and only ever run on reads the device flagged TPS_RES_TIE:
    there two or more candidates are within float64 rounding noise of the best gain, upstream's answer is decided by that noise
    (np.tile([12, 13], 200): 5, where the exact rule says 395), and the only way to give upstream's answer is to repeat
    upstream's arithmetic.  Returns the split index or -1."""
    sig = np.asarray(y, dtype=np.float64).reshape(-1, 1)
    n = sig.shape[0]
    if (n // jump) < 1 or (-(-min_size // jump)) * jump + min_size > n:
        return -1

    def cost(a, b):
        return sig[a:b].var(axis=0).sum() * (b - a)

    whole = cost(0, n)
    best = None
    for b in range(0, n, jump):
        if b >= min_size and n - b >= min_size:
            cand = (whole - cost(0, b) - cost(b, n), b)
            if best is None or cand > best:
                best = cand
    return -1 if best is None else int(best[1])


def resolve_ties(engine, slot: int, res: np.ndarray, n_patterns: int, jump: int = 5, min_size: int = 2) -> int:
    """Reads of `res` whose change-point the device decided by its exact tournament (flags & RES_TIE) get ruptures' float64
    answer instead: their S_w come down (engine.read_sums), y = S_w / P, binseg_l2_float64.  In place; returns how many."""
    if "flags" not in res.dtype.names:
        return 0
    idx = np.nonzero((res["flags"] & RES_TIE) != 0)[0]
    for i in idx:
        s_w = engine.read_sums(slot, int(i), int(res["n_win"][i]))
        res["bkp"][i] = binseg_l2_float64(np.asarray(s_w, dtype=np.float64) / n_patterns, jump, min_size)
    return len(idx)


def _region(tails, begin, end, call):
    """tails / begin / end of the calls that look at one region per read, as the C ABI takes them."""
    tails = np.ascontiguousarray(tails, dtype=np.uint8)
    begin = np.ascontiguousarray(begin, dtype=np.int32)
    end = np.ascontiguousarray(end, dtype=np.int32)
    if not (len(tails) == len(begin) == len(end)):
        raise TopsicleHipError(f"{call}: tails, begin and end must have one entry per read")
    return tails, begin, end


class HipScanner:
    """One context on one MI355X.  Not thread-safe; use one per host thread and device."""

    def __init__(self, device: int = 0, lib_path: str | None = None):
        self.lib = load_library(lib_path)
        n = C.c_int(0)
        rc = self.lib.tps_device_count(C.byref(n))
        if rc != 0 or n.value <= 0:
            raise TopsicleHipError("no MI355X / HIP device visible: " + self._err() + " (topsicle_amd has no CPU fallback)")
        h = C.c_void_p()
        self._check(self.lib.tps_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.patterns: list[str] = []
        self._n = {}
        self._lib_path = lib_path
        self._helpers: list["HipScanner"] = []
        for key, value in debug_options_from_env().items():
            self.debug_option(key, value)

    def debug_option(self, key: str, value: int = 1):
        """tps_ctx_debug_option: diagnostics / tests (event_stride, no_events, force_generic, spans_per_tile, force_pair, so_order,
        wpg, lc_lds, stamps, file_order, no_stride, no_inline_rows, poison).  poison (tests only): 0 = off, 1 .. 255 = the byte every call fills its
        output and scratch buffers with before it runs.  Applies to this context and to the helper contexts it makes afterwards."""
        self._check(self.lib.tps_ctx_debug_option(self._h, key.encode(), int(value)))
        self._debug = getattr(self, "_debug", {})
        self._debug[key] = int(value)
        for h in self._helpers:
            h.debug_option(key, value)

    def stamps(self, slot: int) -> np.ndarray:
        """uint64[n, 16] phase clocks of the slot's last scan (a -DTPS_STAMPS build with the option "stamps" on)."""
        n = self._n[slot]
        out = np.zeros((n, 16), dtype=np.uint64)
        self._check(self.lib.tps_debug_stamps_get(self._h, slot, _ptr(out), n))
        return out

    def helper(self, j: int) -> "HipScanner":
        """The j-th helper context on this context's device (made on first use, closed with this one): with several pattern
        tables per batch (`--telophrase 4 5 6`) every table beyond the first is scanned by a helper that BORROWS this context's
        resident batch (share) and keeps its own table, outputs and stream -- the k passes overlap on the GPU."""
        while len(self._helpers) <= j:
            h = HipScanner(self.device, self._lib_path)
            for key, value in getattr(self, "_debug", {}).items():
                h.debug_option(key, value)
            self._helpers.append(h)
        return self._helpers[j]

    # -- plumbing
    def _err(self) -> str:
        m = self.lib.tps_last_error()
        return m.decode("utf-8", "replace") if m else ""

    def _check(self, rc: int):
        if rc != 0:
            raise TopsicleHipError(f"libtopsicle_hip error {rc}: {self._err()}")

    def close(self):
        for h in getattr(self, "_helpers", []):      # (they borrow this context's batches: they go first)
            h.close()
        self._helpers = []
        if getattr(self, "_h", None):
            self.lib.tps_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def device_info(self) -> str:
        buf = C.create_string_buffer(256)
        self._check(self.lib.tps_device_info(self._h, buf, 256))
        return buf.value.decode()

    # -- pattern table
    def kernel_info(self, slot: int) -> str:
        """'<kernel name> lds=<bytes per workgroup> wgs_per_cu=<n>' of the slot's last scan."""
        buf = C.create_string_buffer(256)
        self._check(self.lib.tps_batch_kernel_info(self._h, slot, buf, 256))
        return buf.value.decode()

    def set_patterns(self, patterns: list[str]):
        if not patterns:
            raise TopsicleHipError("empty pattern list")
        k = len(patterns[0])
        if any(len(p) != k for p in patterns):
            raise TopsicleHipError("all patterns of one table must have the same length")
        blob = "".join(patterns).encode("ascii")
        self._check(self.lib.tps_set_patterns(self._h, blob, len(patterns), k))
        self.patterns = list(patterns)

    def set_patterns_wide(self, patterns: list[str]):
        """Up to WIDE_MAX_PATTERNS patterns of up to WIDE_MAX_K letters (tps_set_patterns_wide): scans then run the wide kernel,
        everything downstream of the scan is unchanged.  Takes narrow tables too; kmer_followers refuses a wide table, kmer_followers_wide
        is the call for it."""
        if not patterns:
            raise TopsicleHipError("empty pattern list")
        k = len(patterns[0])
        if any(len(p) != k for p in patterns):
            raise TopsicleHipError("all patterns of one table must have the same length")
        blob = "".join(patterns).encode("ascii", "replace")
        self._check(self.lib.tps_set_patterns_wide(self._h, blob, len(patterns), k))
        self.patterns = list(patterns)

    # -- resident batches
    def upload(self, slot: int, bases: np.ndarray, offsets: np.ndarray):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        self._check(self.lib.tps_batch_upload(self._h, slot, _ptr(bases), _ptr(offsets), n))
        self._n[slot] = n

    def upload_packed(self, slot: int, seq2: np.ndarray, inv, desc: np.ndarray):
        """A batch the host has packed already (2 bits per base; include/topsicle_hip.h).  Arrays that live in buffers
        from `host_alloc` are copied asynchronously: keep them unchanged until `sync()` / a result download."""
        assert seq2.dtype == np.uint32 and desc.dtype == DESC_DTYPE and (inv is None or inv.dtype == np.uint16)
        n, nw = len(desc), len(seq2)
        assert inv is None or len(inv) == nw
        self._check(self.lib.tps_batch_upload_packed(self._h, slot, _ptr(seq2), _ptr(inv), _ptr(desc), n, nw))
        self._n[slot] = n

    def upload_nib4(self, slot: int, nib: np.ndarray, src: np.ndarray, desc: np.ndarray, n_words: int):
        """A batch of BAM records as stored (seqio.read_batches_packed on BAM input): their 4-bit base codes `nib`, where each read's
        codes are and its strand (`src`, NIB_SRC_DTYPE), the reads' descriptors in the packed layout; a device kernel expands them
        into the slot's packed batch (tps_batch_upload_nib4).  Buffers from `host_alloc` are copied asynchronously, like upload_packed."""
        assert nib.dtype == np.uint8 and src.dtype == NIB_SRC_DTYPE and desc.dtype == DESC_DTYPE and len(src) == len(desc)
        n = len(desc)
        self._check(self.lib.tps_batch_upload_nib4(self._h, slot, _ptr(nib), len(nib), _ptr(src), _ptr(desc), n, int(n_words)))
        self._n[slot] = n

    def share(self, slot: int, src: "HipScanner", src_slot: int):
        """This context's `slot` = the resident batch of `src`'s `src_slot` (same device, no copy): one context per pattern
        table scans one batch at the same time (tps_batch_share)."""
        self._check(self.lib.tps_batch_share(self._h, slot, src._h, src_slot))
        self._n[slot] = src._n[src_slot]

    def host_alloc(self, nbytes: int) -> np.ndarray:
        """Pinned host memory as a uint8 array (freed with the context or by `host_free`)."""
        p = C.c_void_p()
        self._check(self.lib.tps_host_alloc(self._h, int(nbytes), C.byref(p)))
        buf = (C.c_uint8 * max(int(nbytes), 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.uint8, count=int(nbytes))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr: np.ndarray):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None:
            self._check(self.lib.tps_host_free(self._h, C.c_void_p(p)))

    def download_packed(self, slot: int):
        """(seq2, inv, desc) of the slot's resident packed batch (tests / diagnostics)."""
        n = self._n[slot]
        nw = C.c_int64(0)
        self._check(self.lib.tps_batch_download_packed(self._h, slot, None, None, None, n, 0, C.byref(nw)))
        seq2 = np.zeros(nw.value, np.uint32)
        inv = np.zeros(nw.value, np.uint16)
        desc = np.zeros(n, DESC_DTYPE)
        self._check(self.lib.tps_batch_download_packed(self._h, slot, _ptr(seq2), _ptr(inv), _ptr(desc), n, nw.value, None))
        return seq2, inv, desc

    def kmer_followers(self, slot: int, n_fwd: int, follow: int, lo: int = 100, hi: int = 2000, min_len: int = 0, want_hist: bool = True):
        """patterns_vs_match_heatmap's counting (descriptive_plot.py:259-291) on the resident batch:
        (picks uint32[n, 2, n_fwd, pw], hist int64[2, n_fwd, 4**follow + 1] or None)."""
        n = self._n[slot]
        pw = (hi - lo + 31) // 32
        picks = np.zeros((n, 2, n_fwd, pw), dtype=np.uint32)
        hist = np.zeros((2, n_fwd, 4 ** follow + 1), dtype=np.int64) if want_hist else None
        self._check(self.lib.tps_batch_kmer_followers(self._h, slot, n_fwd, follow, lo, hi, min_len, _ptr(picks), picks.size,
                                                      _ptr(hist), 0 if hist is None else hist.size))
        return picks, hist

    def kmer_followers_wide(self, slot: int, n_fwd: int, follow: int, lo: int = 100, hi: int = 2000, min_len: int = 0, want_hist: bool = True):
        """kmer_followers on the table of set_patterns_wide (tps_batch_kmer_followers_wide): up to FOLLOW_WIDE_MAX_FWD k-mers of up to
        WIDE_MAX_K letters, any number of following letters.  (picks uint32[n, 2, n_fwd, pw], hist int64[2, n_fwd, 4**follow + 1] or
        None); the histogram has 4**follow bins and exists for follow <= FOLLOW_HIST_MAX only: ask for picks alone beyond that."""
        if want_hist and follow > FOLLOW_HIST_MAX:
            raise TopsicleHipError(f"the followers histogram has 4**follow bins: follow must be 0..{FOLLOW_HIST_MAX} with it, got {follow} (want_hist=False returns the picks alone)")
        n = self._n[slot]
        pw = max((hi - lo + 31) // 32, 0)              # (what the library refuses it refuses itself: n_fwd, follow, the range)
        picks = np.zeros((n, 2, max(n_fwd, 0), pw), dtype=np.uint32)
        hist = np.zeros((2, max(n_fwd, 0), 4 ** max(follow, 0) + 1), dtype=np.int64) if want_hist else None
        self._check(self.lib.tps_batch_kmer_followers_wide(self._h, slot, n_fwd, follow, lo, hi, min_len, _ptr(picks), picks.size,
                                                           _ptr(hist), 0 if hist is None else hist.size))
        return picks, hist

    def motif_census(self, slot: int, u_min: int = 4, u_max: int = 32, lo: int = 0, hi: int = 1000, min_len: int = 0, want_counts: bool = False):
        """What repeats at the read ends of the resident batch, no pattern table needed (tps_batch_motif_census; the rule is in
        include/topsicle_hip.h): hits MOTIF_HIT_DTYPE[n, 2] -- per read and end (0 = the read's start, 1 = the start of its reverse
        complement) the period with the most recurring 8-mers, that count, the longest run and the unit it starts with -- and, with
        want_counts, counts int32[n, 2, u_max - u_min + 1] of every period (None otherwise)."""
        n = self._n[slot]
        hits = np.zeros((n, 2), dtype=MOTIF_HIT_DTYPE)
        counts = np.zeros((n, 2, max(u_max - u_min + 1, 0)), dtype=np.int32) if want_counts else None      # (a bad period range is the library's to refuse)
        self._check(self.lib.tps_batch_motif_census(self._h, slot, u_min, u_max, lo, hi, min_len, _ptr(hits), hits.size,
                                                    _ptr(counts), 0 if counts is None else counts.size))
        return hits, counts

    def variant_census(self, slot: int, unit: str, tails, begin, end, bin: int = 500, n_bins: int = 40, want_profile: bool = True):
        """What the tract [begin, end) of every read of the resident batch is made of, against the primitive unit `unit` (a string
        of ACGT, 2 .. 32 letters; tps_batch_variant_census, the rule is in include/topsicle_hip.h; names and columns:
        topsicle_amd.variants): (counts uint32[n, 2 + 4m], profile int64[n_bins, 2 + 4m] or None).  Column 0 = positions examined,
        1 = canonical, 2 + 4p + c = letter c (ACTG = 0123) seen at place p of the unit.  No pattern table needed; the slot's scan
        outputs stay as they are."""
        from . import variants
        code, m = variants.unit_code(unit)
        n = self._n[slot]
        tails, begin, end = _region(tails, begin, end, "variant_census")
        cols = 2 + 4 * m
        counts = np.zeros((n, cols), dtype=np.uint32)
        profile = np.zeros((max(n_bins, 0), cols), dtype=np.int64) if want_profile else None      # (a bad bin count is the library's to refuse)
        self._check(self.lib.tps_batch_variant_census(self._h, slot, code, m, _ptr(tails), _ptr(begin), _ptr(end), len(tails), bin, n_bins,
                                                      _ptr(counts), counts.size, _ptr(profile), 0 if profile is None else profile.size))
        return counts, profile

    def tract_map(self, slot: int, unit: str, block: int = 64, min_hits: int = 20, gap: int = 1, min_blocks: int = 2, max_tracts: int = 8):
        """Where in the whole reads of the resident batch repeats of the primitive unit `unit` (a string of ACGT, 4 .. 32 letters)
        lie, on either strand (tps_batch_tract_map, the rule is in include/topsicle_hip.h; classes and files: topsicle_amd.tracts):
        (tracts TRACT_DTYPE[n, 2, max_tracts], found int32[n, 2], totals uint32[n, 4]).  Strand 0 is the unit as given, strand 1 its
        reverse complement; found is the true number of tracts, of which tracts holds the first max_tracts.  No pattern table
        needed; the slot's scan outputs stay as they are."""
        from . import variants
        code, m = variants.unit_code(unit)
        n = self._n[slot]
        mt = max_tracts if TRACT_MAX_TRACTS_RANGE[0] <= max_tracts <= TRACT_MAX_TRACTS_RANGE[1] else 1      # (a bad count is the library's to refuse)
        tracts = np.zeros((n, 2, mt), dtype=TRACT_DTYPE)
        found = np.zeros((n, 2), dtype=np.int32)
        totals = np.zeros((n, 4), dtype=np.uint32)
        self._check(self.lib.tps_batch_tract_map(self._h, slot, code, m, block, min_hits, gap, min_blocks, max_tracts,
                                                 _ptr(tracts), n * 2 * max_tracts, _ptr(found), found.size, _ptr(totals), totals.size))
        return tracts, found, totals

    def end_sketch(self, slot: int, unit: str, tails, begin, end, k: int = 12, buckets: int = 256):
        """A sketch of the window [begin, end) of every read of the resident batch, telomere first (tails: 0 = the read, 1 = its
        reverse complement): the smallest hash per bucket over the k-mers that hold no word of the telomere repeat `unit` (a
        primitive word of ACGT, 4 .. 32 letters; tps_batch_end_sketch, the rule is in include/topsicle_hip.h; groups and files:
        topsicle_amd.ends): (sketch uint32[n, buckets], kept uint32[n]).  An empty bucket holds ENDS_EMPTY.  No pattern table
        needed; the slot's scan outputs stay as they are."""
        from . import variants
        code, m = variants.unit_code(unit)
        n = self._n[slot]
        tails, begin, end = _region(tails, begin, end, "end_sketch")
        nb = buckets if buckets in ENDS_BUCKETS else ENDS_BUCKETS[0]          # (a bad count is the library's to refuse)
        sketch = np.zeros((n, nb), dtype=np.uint32)
        kept = np.zeros(n, dtype=np.uint32)
        self._check(self.lib.tps_batch_end_sketch(self._h, slot, code, m, k, buckets, _ptr(tails), _ptr(begin), _ptr(end), len(tails),
                                                  _ptr(sketch), n * buckets, _ptr(kept), kept.size))
        return sketch, kept

    def sketch_links(self, sketch, min_match: int = 6, max_links: int = 32):
        """All pairs of the rows of `sketch` (uint32[n, buckets], as end_sketch returns them; tps_sketch_links): (degree int32[n],
        links int32[n, max_links], matches int32[n, max_links]) -- per row i the true number of rows j > i that share at least
        min_match non-empty buckets with it, the smallest such j in ascending order (-1 behind them) and their match counts.  Needs
        no resident batch."""
        sketch = np.ascontiguousarray(sketch, dtype=np.uint32)
        if sketch.ndim != 2:
            raise TopsicleHipError("sketch_links: sketch must be a 2-d array")
        n, b = sketch.shape
        ml = max_links if 1 <= max_links <= LINKS_MAX_LINKS else 1            # (a bad count is the library's to refuse)
        degree = np.zeros(n, dtype=np.int32)
        links = np.full((n, ml), -1, dtype=np.int32)
        matches = np.zeros((n, ml), dtype=np.int32)
        self._check(self.lib.tps_sketch_links(self._h, _ptr(sketch), n, b, sketch.size, min_match, max_links, _ptr(degree), degree.size,
                                              _ptr(links), n * max_links, _ptr(matches), n * max_links))
        return degree, links, matches

    def end_window(self, slot: int, unit: str, tails, begin, end, k: int = 12, span: int = 2000):
        """The kept window of every read of the resident batch, position by position (tps_batch_end_window; the rule is in
        include/topsicle_hip.h): the window [begin, end) end_sketch hashes, as (codes uint32[n, (span + 15) // 16], keep
        uint32[n, (span + 31) // 32]) -- 2-bit letters, 16 per dword, and one bit per position whose k-mer the sketch keeps.  No
        window may be longer than span (k .. 4096).  No pattern table needed; the slot's scan outputs stay as they are."""
        from . import variants
        code, m = variants.unit_code(unit)
        n = self._n[slot]
        tails, begin, end = _region(tails, begin, end, "end_window")
        sp = span if 1 <= span <= ANCHOR_MAX_SPAN else 1                       # (a bad span is the library's to refuse)
        codes = np.zeros((n, (sp + 15) // 16), dtype=np.uint32)
        keep = np.zeros((n, (sp + 31) // 32), dtype=np.uint32)
        self._check(self.lib.tps_batch_end_window(self._h, slot, code, m, k, _ptr(tails), _ptr(begin), _ptr(end), len(tails), span,
                                                  _ptr(codes), codes.size, _ptr(keep), keep.size))
        return codes, keep

    def anchor_offsets(self, codes, keep, length, ref, span: int, k: int = 12):
        """The offset of window i against window ref[i] by votes on their diagonals (tps_window_offsets): rows as end_window returns
        them, length[i] letters each, ref[i] < 0 for a row without a reference: (offset int32[n], votes int32[n], second
        int32[n]) -- the lower median of the best 128 diagonals in window coordinates, the votes there, and the best count two
        coarse bins or more away.  Needs no resident batch."""
        codes = np.ascontiguousarray(codes, dtype=np.uint32)
        keep = np.ascontiguousarray(keep, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.int32)
        ref = np.ascontiguousarray(ref, dtype=np.int32)
        n = len(ref)
        sp = span if 1 <= span <= ANCHOR_MAX_SPAN else 1
        if codes.shape != (n, (sp + 15) // 16) or keep.shape != (n, (sp + 31) // 32) or len(length) != n:
            raise TopsicleHipError("anchor_offsets: codes, keep, length and ref must hold one row of `span` letters per window")
        offset, votes, second = (np.zeros(n, dtype=np.int32) for _ in range(3))
        self._check(self.lib.tps_window_offsets(self._h, _ptr(codes), _ptr(keep), _ptr(length), _ptr(ref), n, span, k,
                                                _ptr(offset), _ptr(votes), _ptr(second), n))
        return offset, votes, second

    def place_windows(self, codes, keep, length, ref_codes, ref_keep, ref_length, span: int, k: int = 12, max_occ: int = 16):
        """n query windows placed on R reference windows (tps_window_place; the rule is in include/topsicle_hip.h): both sets as rows
        the way end_window returns them, length[i] letters each.  Returns (ref, total, runner_ref, runner, offset, votes, second),
        int32[n] each -- the reference row with the most matching k-mers and their number, the same for the best other row, and the
        offset of the window against that reference row's with its votes and runner-up as anchor_offsets gives them.  A k-mer with
        more than max_occ entries over all reference rows takes no part.  Needs no resident batch and no pattern table."""
        codes = np.ascontiguousarray(codes, dtype=np.uint32)
        keep = np.ascontiguousarray(keep, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.int32)
        ref_codes = np.ascontiguousarray(ref_codes, dtype=np.uint32)
        ref_keep = np.ascontiguousarray(ref_keep, dtype=np.uint32)
        ref_length = np.ascontiguousarray(ref_length, dtype=np.int32)
        n, n_ref = len(length), len(ref_length)
        sp = span if 1 <= span <= ANCHOR_MAX_SPAN else 1                       # (a bad span is the library's to refuse)
        cdw, kdw = (sp + 15) // 16, (sp + 31) // 32
        if codes.shape != (n, cdw) or keep.shape != (n, kdw) or ref_codes.shape != (n_ref, cdw) or ref_keep.shape != (n_ref, kdw):
            raise TopsicleHipError("place_windows: codes / keep and ref_codes / ref_keep must hold one row of `span` letters per window")
        out = [np.zeros(n, dtype=np.int32) for _ in range(7)]
        self._check(self.lib.tps_window_place(self._h, _ptr(codes), codes.size, _ptr(keep), keep.size, _ptr(length), n, _ptr(ref_codes), ref_codes.size,
                                              _ptr(ref_keep), ref_keep.size, _ptr(ref_length), n_ref, span, k, max_occ, *[_ptr(o) for o in out], n))
        return tuple(out)

    def align_windows(self, codes, length, ref_codes, ref_length, ref, centre, span: int, cols: bool = True, pile_row=None, n_pile: int = 0):
        """n query windows aligned base by base against reference windows inside a band of 64 diagonals (tps_window_align; the rule
        is in include/topsicle_hip.h): both sets as codes rows the way end_window returns them, length[i] / ref_length[r] letters
        each; ref[i] = the reference row of query i (< 0: none), centre[i] = the diagonal the band sits on (anchor_offsets' offset).
        Returns (stat int32[n, 6], cols uint16[n, span] or None, pile int32[n_pile, span, 13] or None): dist, q_begin, q_end,
        r_begin, r_end and flags (1 = no alignment, 2 = the path touched the band's edge); the state of every reference column;
        and, with pile_row (the pile row a pair counts for, < 0: none) and n_pile > 0, the votes of the unflagged pairs per pile
        row and column.  Needs no resident batch and no pattern table."""
        codes = np.ascontiguousarray(codes, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.int32)
        ref_codes = np.ascontiguousarray(ref_codes, dtype=np.uint32)
        ref_length = np.ascontiguousarray(ref_length, dtype=np.int32)
        ref = np.ascontiguousarray(ref, dtype=np.int32)
        centre = np.ascontiguousarray(centre, dtype=np.int32)
        n, n_ref = len(length), len(ref_length)
        sp = span if 1 <= span <= ALIGN_MAX_SPAN else 1                        # (a bad span is the library's to refuse)
        cdw = (sp + 15) // 16
        if codes.shape != (n, cdw) or ref_codes.shape != (n_ref, cdw) or len(ref) != n or len(centre) != n:
            raise TopsicleHipError("align_windows: codes / ref_codes must hold one row of `span` letters per window, ref and centre one entry per query")
        if pile_row is not None:
            pile_row = np.ascontiguousarray(pile_row, dtype=np.int32)
            if len(pile_row) != n:
                raise TopsicleHipError("align_windows: pile_row must hold one entry per query")
        stat = np.zeros((n, ALIGN_STATS), dtype=np.int32)
        out_cols = np.zeros((n, sp), dtype=np.uint16) if cols else None
        pile = np.zeros((n_pile, sp, ALIGN_PILE), dtype=np.int32) if n_pile > 0 else None
        self._check(self.lib.tps_window_align(self._h, _ptr(codes), codes.size, _ptr(length), n, _ptr(ref_codes), ref_codes.size, _ptr(ref_length), n_ref,
                                              _ptr(ref), _ptr(centre), span, _ptr(stat), stat.size, _ptr(out_cols), 0 if out_cols is None else out_cols.size,
                                              _ptr(pile_row), _ptr(pile), n_pile, 0 if pile is None else pile.size))
        return stat, out_cols, pile

    def adapter_find(self, slot: int, patterns, tails, begin, end):
        """Every sequence of `patterns` (strings of ACGT, 12 .. 64 letters, at most 64 of them, telomere first like the region)
        searched approximately in the region [begin, end) of every read of the resident batch (tails: 0 = the read, 1 = its reverse
        complement; at most 1024 letters; tps_batch_adapter_find, the rule is in include/topsicle_hip.h; names and files:
        topsicle_amd.adapters): (dist uint16[n, P], end uint16[n, P]) -- the smallest edit distance between the pattern and any
        substring of the region, and the smallest end of such a substring, relative to begin.  No pattern table needed; the slot's
        scan outputs stay as they are."""
        from . import adapters
        codes, lens = adapters.pattern_codes(patterns)
        n = self._n[slot]
        tails, begin, end = _region(tails, begin, end, "adapter_find")
        hits = np.zeros((n, len(lens), 2), dtype=np.uint16)
        self._check(self.lib.tps_batch_adapter_find(self._h, slot, _ptr(codes), _ptr(lens), len(lens), _ptr(tails), _ptr(begin), _ptr(end), len(tails),
                                                    _ptr(hits), hits.size))
        return hits[:, :, 0].copy(), hits[:, :, 1].copy()

    def boundary_refine(self, slot: int, unit: str, tails, begin, end, at, hit: int = 2, miss: int = 1, sep: int = 200):
        """The boundary of the telomere tract at base resolution in the region [begin, end) of every read of the resident batch
        (tails: 0 = the read, 1 = its reverse complement; at most 65 536 letters), and what supports it: one change point on the
        per-position hits of the primitive unit `unit` (a string of ACGT, 4 .. 32 letters), a hit worth +hit, any other position
        -miss (tps_batch_boundary_refine, the rule is in include/topsicle_hip.h; classes and files: topsicle_amd.refine):
        REFINE_DTYPE[n] -- pos and its score, the drop from there to the region's end, the score at the boundary `at` the caller has
        called, the hits on either side, and the best boundary at least `sep` positions away.  No pattern table needed; the slot's
        scan outputs stay as they are."""
        from . import variants
        code, m = variants.unit_code(unit)
        n = self._n[slot]
        tails, begin, end = _region(tails, begin, end, "boundary_refine")
        at = np.ascontiguousarray(at, dtype=np.int32)
        if len(at) != len(tails):
            raise TopsicleHipError("boundary_refine: at must have one entry per read")
        out = np.zeros(n, dtype=REFINE_DTYPE)
        self._check(self.lib.tps_batch_boundary_refine(self._h, slot, code, m, _ptr(tails), _ptr(begin), _ptr(end), _ptr(at), len(tails), hit, miss, sep,
                                                       _ptr(out), out.size))
        return out

    def mod_profile(self, slot: int, tails, begin, end, origin, mod_off, delta, prob, w: int = 500, nb0: int = 2, nb1: int = 8, hi: int = 205, lo: int = 50):
        """The calls of one base modification (BAM MM / ML tags: seqio.bam_mods gives mod_off / delta / prob) put on the reads of the
        resident batch and binned against `origin` in the region [begin, end) of every read (tails: 0 = the read, 1 = counted from its
        far end; at most 16 384 bases, inside the nb0 bins of w bases in front of origin and the nb1 behind it): (MOD_ROW_DTYPE[n],
        MOD_BIN_DTYPE[n, nb0 + nb1]) -- per read its C's, entries, those beyond the last C, in the region, off a CpG, and per bin the
        CpGs of the sequence, the calls on them, their prob sum, those >= hi and those <= lo (tps_batch_mod_profile, the rule is in
        include/topsicle_hip.h; the files: topsicle_amd.methyl).  No pattern table needed; the slot's scan outputs stay as they are."""
        n = self._n[slot]
        tails, begin, end = _region(tails, begin, end, "mod_profile")
        origin = np.ascontiguousarray(origin, dtype=np.int32)
        mod_off = np.ascontiguousarray(mod_off, dtype=np.int64)
        delta = np.ascontiguousarray(delta, dtype=np.uint32)
        prob = np.ascontiguousarray(prob, dtype=np.uint8)
        if len(origin) != len(tails) or len(mod_off) != len(tails) + 1 or len(delta) != len(prob):
            raise TopsicleHipError("mod_profile: origin must have one entry per read, mod_off one more, delta and prob the same number")
        nb = max(int(nb0) + int(nb1), 0)
        rows = np.zeros(n, dtype=MOD_ROW_DTYPE)
        bins = np.zeros((n, nb), dtype=MOD_BIN_DTYPE)
        self._check(self.lib.tps_batch_mod_profile(self._h, slot, _ptr(tails), _ptr(begin), _ptr(end), _ptr(origin), len(tails), _ptr(mod_off), _ptr(delta),
                                                   _ptr(prob), len(delta), int(w), int(nb0), int(nb1), int(hi), int(lo), _ptr(rows), rows.size, _ptr(bins), bins.size))
        return rows, bins

    def set_tails(self, slot: int, tails: np.ndarray):
        tails = np.ascontiguousarray(tails, dtype=np.uint8)
        assert len(tails) == self._n[slot]
        self._check(self.lib.tps_batch_set_tails(self._h, slot, _ptr(tails)))

    def scan(self, slot: int, prm: Params):
        self._check(self.lib.tps_batch_scan(self._h, slot, C.byref(prm)))

    def sync(self):
        self._check(self.lib.tps_sync(self._h))

    def results(self, slot: int) -> np.ndarray:
        n = self._n[slot]
        out = np.zeros(n, dtype=RESULT_DTYPE)
        self._check(self.lib.tps_batch_results(self._h, slot, _ptr(out), n))
        return out

    def window_offsets(self, slot: int) -> np.ndarray:
        n = self._n[slot]
        out = np.zeros(n + 1, dtype=np.int64)
        self._check(self.lib.tps_batch_window_offsets(self._h, slot, _ptr(out), n + 1))
        return out

    def window_sums(self, slot: int) -> tuple[np.ndarray, np.ndarray]:
        off = self.window_offsets(slot)
        out = np.zeros(int(off[-1]), dtype=np.int32)
        self._check(self.lib.tps_batch_window_sums(self._h, slot, _ptr(out), len(out)))
        return out, off

    def read_sums(self, slot: int, read: int, n_win: int) -> np.ndarray:
        """S_w of one read of the slot's last scan (any scan that ran the window step)."""
        out = np.zeros(int(n_win), dtype=np.int32)
        self._check(self.lib.tps_batch_read_sums(self._h, slot, int(read), _ptr(out), len(out)))
        return out

    def window_raw(self, slot: int) -> tuple[np.ndarray, np.ndarray]:
        off = self.window_offsets(slot)
        p = len(self.patterns)
        out = np.zeros(int(off[-1]) * p, dtype=np.uint8)
        self._check(self.lib.tps_batch_window_raw(self._h, slot, _ptr(out), len(out)))
        return out.reshape(-1, p), off

    def raw_to_fd(self, slot: int, reads: np.ndarray, fd: int, file_off: int) -> tuple[int, int]:
        """The raw rows of `reads` (ascending read indices of the slot's batch) of the last scan, back to back at byte `file_off`
        of `fd`: device -> pinned pieces -> pwritev inside the library (tps_batch_raw_to_fd).  Returns (bytes written, their
        CRC-32 -- libtopsicle_io.so's carry-less-multiplication CRC runs over the pieces as they are written)."""
        reads = np.ascontiguousarray(reads, dtype=np.int64)
        crc, nbytes = C.c_uint32(0), C.c_int64(0)
        self._check(self.lib.tps_batch_raw_to_fd(self._h, slot, _ptr(reads), len(reads), int(fd), int(file_off), _crc32_callback(),
                                                 C.byref(crc), C.byref(nbytes)))
        return nbytes.value, crc.value

    def batch_trc_counts(self, slot: int) -> tuple[np.ndarray, np.ndarray]:
        n, p = self._n[slot], len(self.patterns)
        cs = np.zeros((n, p), dtype=np.int32)
        ce = np.zeros((n, p), dtype=np.int32)
        self._check(self.lib.tps_batch_trc_counts(self._h, slot, _ptr(cs), _ptr(ce), n))
        return cs, ce

    # -- one-shot calls
    def trc_counts(self, bases, offsets, no_bp: int = 1000):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n, p = len(offsets) - 1, len(self.patterns)
        cs = np.zeros((n, p), dtype=np.int32)
        ce = np.zeros((n, p), dtype=np.int32)
        self._check(self.lib.tps_trc_counts(self._h, _ptr(bases), _ptr(offsets), n, no_bp, _ptr(cs), _ptr(ce)))
        return cs, ce

    def window_counts(self, bases, offsets, tails, window, slide, trimfirst, maxlen, raw=False):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        tails = np.ascontiguousarray(tails, dtype=np.uint8)
        n, p = len(offsets) - 1, len(self.patterns)
        lens = np.diff(offsets)
        nw = np.array([window_count(int(x), window, slide, trimfirst, maxlen) for x in lens], dtype=np.int64)
        win_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(nw, out=win_off[1:])
        sums = np.zeros(int(win_off[-1]), dtype=np.int32)
        rawbuf = np.zeros(int(win_off[-1]) * p, dtype=np.uint8) if raw else None
        self._check(self.lib.tps_window_counts(self._h, _ptr(bases), _ptr(offsets), _ptr(tails), n, window, slide,
                                               trimfirst, maxlen, _ptr(win_off), _ptr(sums), _ptr(rawbuf)))
        return sums, win_off, (rawbuf.reshape(-1, p) if raw else None)

    def binseg_l2(self, sums, win_off, n_patterns, jump=5, min_size=2):
        sums = np.ascontiguousarray(sums, dtype=np.int32)
        win_off = np.ascontiguousarray(win_off, dtype=np.int64)
        n = len(win_off) - 1
        bkp = np.full(n, -1, dtype=np.int32)
        gain = np.zeros(n, dtype=np.float64)
        tie = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.tps_binseg_l2_ties(self._h, _ptr(sums), _ptr(win_off), n, n_patterns, jump, min_size, _ptr(bkp), _ptr(gain), _ptr(tie)))
        for i in np.nonzero(tie)[0]:                   # float64 cannot separate the best candidates: ruptures' own arithmetic decides
            bkp[i] = binseg_l2_float64(sums[win_off[i]:win_off[i + 1]].astype(np.float64) / n_patterns, jump, min_size)
        return bkp, gain

    # -- measurement
    def kernel_time_ms(self) -> tuple[int, float, float]:
        n, tot, mean = C.c_int32(0), C.c_double(0), C.c_double(0)
        self._check(self.lib.tps_kernel_time_ms(self._h, C.byref(n), C.byref(tot), C.byref(mean)))
        return n.value, tot.value, mean.value

    def kernel_time_reset(self):
        self._check(self.lib.tps_kernel_time_reset(self._h))
