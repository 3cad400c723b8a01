/*
 * topsicle_hip.h -- C ABI of libtopsicle_hip.so: the MI355X (gfx950) implementation of
 * Topsicle's per-read hot path.
 *
 * The reference (jaeyoungchoilab/Topsicle) has NO plugin / FFI seam: the path is a chain of
 * plain Python calls inside Topsicle/allsteps.py, driven by Topsicle/main.py:52-154.  This
 * header is therefore the boundary a maintainer would bind (ctypes stub in INTEGRATION.md);
 * each entry point names the reference code it replaces (file:line relative to the reference
 * root).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no exceptions cross the boundary.
 *   - every function returns 0 on success or a negative TPS_E_* code; tps_last_error() gives
 *     the message of the last failure on the calling thread.
 *   - the caller allocates and owns every host buffer; the library keeps no host pointer
 *     after a call returns -- with ONE exception: uploads from buffers obtained with tps_host_alloc
 *     (pinned memory) are asynchronous on the context's stream, and those buffers must not be
 *     rewritten or freed before the next tps_sync (or blocking download) on that context.
 *     Device memory is owned by the context.
 *   - one context per (host thread, device); a context is not thread-safe, distinct contexts
 *     are independent.  There is NO CPU fallback: creating a context without a usable GPU
 *     fails with TPS_E_NO_DEVICE.
 *   - reads are passed as ONE concatenated ASCII byte string plus n+1 offsets (any case,
 *     any IUPAC letter; only A/C/G/T in either case can match, exactly like the reference's
 *     .upper() + literal regex) -- or already 2-bit packed (tps_batch_upload_packed).  Either way a batch is
 *     RESIDENT in HBM in the packed format below; the scan kernels read nothing else.
 *
 * Packed batch format (what the reference's Bio.SeqIO records, allsteps.py:127-149, become on this path)
 *   seq2   uint32 words, 16 bases per word, base j of a word in bits [2j, 2j+1]; code = (ASCII >> 1) & 3:
 *          A,a = 0   C,c = 1   T,t = 2   G,g = 3
 *   inv    uint16 per word: bit j set = base j of the word is not one of acgtACGT (it never matches)
 *   desc   one tps_read_desc per read; a read starts on a 16-byte boundary (word_off is a multiple of 4) and the words
 *          up to the next such boundary after its last base are zero in seq2 and inv
 *   3 bits per base instead of 8 across PCIe; libtopsicle_io.so's reader emits this format directly.
 */
#ifndef TOPSICLE_HIP_H
#define TOPSICLE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPS_ABI_VERSION 4

/* error codes */
#define TPS_OK            0
#define TPS_E_NO_DEVICE  -1   /* no HIP device / device index out of range              */
#define TPS_E_HIP        -2   /* a HIP runtime call failed (message has the HIP error)  */
#define TPS_E_ARG        -3   /* invalid argument                                        */
#define TPS_E_PATTERN    -4   /* pattern table not set / unsupported (non-ACGT, k>15, P>31; wide tables: k>32, P>64) */
#define TPS_E_CAPACITY   -5   /* parameter combination does not fit the kernel's LDS plan */
#define TPS_E_STATE      -6   /* call order (e.g. scan before upload)                    */

/* limits of this build */
#define TPS_MAX_K         15  /* k-mer length: 4^k-entry LDS table up to TPS_DIRECT_K, a perfect-hash table above */
#define TPS_DIRECT_K      7
#define TPS_MAX_PATTERNS 31   /* patterns in one table (bit 31 of the mask is a flag)       */
#define TPS_WIDE_MAX_K        32  /* wide tables (tps_set_patterns_wide): a k-mer's 2-bit code fits 64 bits          */
#define TPS_WIDE_MAX_PATTERNS 64  /* ... and a 32-letter motif has 64 patterns at every k                            */

/* flags for tps_params.flags */
#define TPS_F_STEP1      1u   /* run the TRC step (a3) and choose tail / pass per read       */
#define TPS_F_WINDOWS    2u   /* run the sliding-window count step (a5) on passing reads     */
#define TPS_F_BINSEG     4u   /* run the single-split change-point step (a6) in the same launch */
#define TPS_F_STORE_SUMS 8u   /* make S_w downloadable (tps_batch_window_sums hands out int32)  */
#define TPS_F_STORE_RAW 16u   /* keep c'_p per window and pattern (u8) -- rawCountPattern (a7) */
#define TPS_F_TAILS_IN  32u   /* without STEP1: tails[] and pass come from the caller         */

typedef struct tps_ctx tps_ctx;

/* One read of a packed batch (16 bytes). */
typedef struct tps_read_desc {
    int64_t  word_off;    /* index of the read's first word in seq2 / inv; a multiple of 4            */
    int32_t  len;         /* bases                                                                     */
    uint32_t flags;       /* TPS_RD_*                                                                  */
} tps_read_desc;
#define TPS_RD_HAS_INVALID 1u   /* the read holds at least one base that is not acgtACGT (inv is consulted) */

/* Where one read of a nib4 batch (tps_batch_upload_nib4) keeps its bases: BAM's 4-bit codes as stored (SAMv1 4.2.3,
 * "=ACMGRSVTWYHKDBN" = 0..15, two per byte, high nibble first), from byte `off` (a multiple of 16) of the nibble buffer. */
typedef struct tps_nib_src {
    int64_t  off;         /* byte offset of the read's first nibble pair in the nibble buffer; a multiple of 16            */
    uint32_t flags;       /* TPS_NIB_*                                                                                       */
    uint32_t reserved;
} tps_nib_src;
#define TPS_NIB_REVERSE 1u      /* the record is reverse-strand (BAM flag 0x10): the read is the reverse complement of the codes */

/* Parameters of one scan.  Names follow the reference CLI (Topsicle/main.py:319-334). */
typedef struct tps_params {
    int32_t no_bp;        /* step-1 tail length; reference hard-codes 1000 (main.py:57)        */
    int32_t min_len;      /* --minSeqLength: keep reads with L >  min_len (allsteps.py:175)    */
    int32_t min_count;    /* keep reads whose best count > min_count; the host derives it from
                             --cutoff so that count/(no_bp/len(pattern)) > cutoff in float64  */
    int32_t window;       /* --windowSize W (window text is W-1 chars, allsteps.py:221-224)    */
    int32_t slide;        /* --slide s                                                         */
    int32_t trimfirst;    /* --trimfirst t                                                     */
    int32_t maxlen;       /* --maxlengthtelo M                                                 */
    int32_t jump;         /* ruptures Binseg jump (5)                                          */
    int32_t min_size;     /* ruptures Binseg min_size (2)                                      */
    uint32_t flags;       /* TPS_F_*                                                           */
} tps_params;

/* Per-read result of a scan (48 bytes; ABI 3 added `flags`). */
typedef struct tps_read_result {
    int32_t best_start;      /* max_p count in the first no_bp bases                (a3)      */
    int32_t best_start_idx;  /* first pattern index reaching it (allsteps.py:190)             */
    int32_t best_end;        /* max_p count in the reversed last no_bp bases                  */
    int32_t best_end_idx;    /* first pattern index reaching it (allsteps.py:191)             */
    int32_t tail;            /* 0 = forward, 1 = reverse (allsteps.py:193-198)                */
    int32_t pass;            /* 1 if L > min_len and best count > min_count                   */
    int32_t n_win;           /* windows of the chosen tail (0 if not scanned)                 */
    int32_t bkp;             /* best split index, -1 if none admissible / not run   (a6)      */
    double  gain;            /* l2 gain of that split on y = S/P (float64, informational)     */
    uint32_t flags;          /* TPS_RES_*                                                     */
    uint32_t reserved;
} tps_read_result;
/* The change-point was decided by the exact integer tournament: two or more candidates lay within float64 rounding noise of
 * the best gain (a constant signal; exact rational ties).  ruptures compares float64 gains there (allsteps.py:310-311), so
 * its answer is a matter of rounding noise, not of the data: a caller that wants THAT answer downloads the read's S_w
 * (tps_batch_read_sums) and repeats ruptures' float64 arithmetic on it -- a handful of reads at most; topsicle_amd does
 * (hiplib.HipScanner.resolve_ties).  bkp itself holds the exact rule's answer: ties -> the larger index. */
#define TPS_RES_TIE 1u

/* ---- context ------------------------------------------------------------------------- */
int  tps_abi_version(void);
int  tps_device_count(int* n);
int  tps_ctx_create(int device, tps_ctx** out);
int  tps_ctx_destroy(tps_ctx* ctx);
const char* tps_last_error(void);

/* Replaces patterns_to_search's consumer side (allsteps.py:167-168, 249-250, 378-379): the
 * compiled regex list.  `pats` holds P strings of k ASCII letters back to back, in reference
 * order (sorted k-mers then their complements, allsteps.py:104-120); order defines pattern
 * indices (first-max tie-break, raw count column order). */
int  tps_set_patterns(tps_ctx* ctx, const char* pats, int32_t n_patterns, int32_t k);
/* The same for tables beyond TPS_MAX_K / TPS_MAX_PATTERNS: 1 <= k <= TPS_WIDE_MAX_K letters, 1 <= n_patterns <= TPS_WIDE_MAX_PATTERNS
 * -- the reference's defaults (k = len - 2, 2 len patterns: Topsicle/main.py:189-193) for every motif of 16 to 32 letters.  Any list
 * of equal-length ACGT strings in reference order is legal: duplicates, k-mers that overlap themselves, narrow tables too.  While a
 * wide table is current tps_batch_scan launches ONE kernel for every slide and flag combination (tps_scan_kernel_wide: 64-bit k-mer
 * codes, a hash of the distinct codes, counts per window by sliding) and every call downstream of the scan works unchanged; the
 * one-shot calls scan with it too.  tps_batch_kmer_followers keeps n_fwd <= 15 and refuses a wide table: its counterpart for the
 * tables set here is tps_batch_kmer_followers_wide (n_fwd <= 32, any number of following letters).  A window that can hold more
 * than 255 occurrences of a k-mer ((window - 1) / k > 255), or a window / step-1 head of more than 32768 bases, is TPS_E_CAPACITY.
 * In practice the LDS plan refuses (TPS_E_CAPACITY as well) long before 32768: a tile holds max(4096, window - 1, no_bp) positions,
 * rounded up to 64, four waves share a workgroup, and the workgroup's budget is min(LDS per block, 160 KB).  Where that ends depends
 * on how many distinct k-mers of the table can overlap themselves (have a period below k: a k-mer whose first and last letters agree
 * is one): at the MI355X's 160 KB the largest step-1 head accepted is 25280 bases with none (e.g. the table A, T), 24896 with four
 * (ACAC... at k = 16) and 24000 with fourteen (the 23-letter motif at k = 21); 64 bases more is refused.  At a 64 KB budget the
 * same three tables stop at 7424, 7040 and 6080.  At 160 KB a window meets the counters' limit first (k <= 32: window - 1 <= 8191).
 * The next tps_set_patterns makes the narrow kernels current again; either call re-plans every resident batch. */
int  tps_set_patterns_wide(tps_ctx* ctx, const char* pats, int32_t n_patterns, int32_t k);

/* ---- resident batch (throughput path) ------------------------------------------------ */
/* Copy a batch of reads into HBM.  `slot` (0..TPS_MAX_SLOTS-1) names one resident batch so
 * several can be kept and scanned in turn.  Replaces the per-call file parse of
 * unzip_file/SeqIO.parse (allsteps.py:127-149, 174, 257) with one upload per batch. */
#define TPS_MAX_SLOTS 16
int  tps_batch_upload(tps_ctx* ctx, int32_t slot, const uint8_t* bases, const int64_t* offsets,
                      int64_t n_reads);
/* The same for a batch the host has already packed (format above): seq2[n_words], inv[n_words] (NULL = no read has an
 * invalid base), desc[n_reads].  Three bits per base cross PCIe instead of eight.  Replaces allsteps.py:127-149 +
 * main.py:68-86 (the parse that feeds every later step) together with libtopsicle_io.so's tps_reader_next_packed.
 * Buffers obtained from tps_host_alloc are pinned: the copies then run asynchronously on the context's stream and the
 * call returns at once -- the caller must keep those buffers unchanged until tps_sync (or any result download of the
 * slot) has returned; ordinary memory is copied before the call returns. */
int  tps_batch_upload_packed(tps_ctx* ctx, int32_t slot, const uint32_t* seq2, const uint16_t* inv,
                             const tps_read_desc* desc, int64_t n_reads, int64_t n_words);
/* The same for a batch of BAM records (libtopsicle_io.so's tps_reader_next_nib4): nib[nib_bytes] holds each read's 4-bit codes as
 * stored, src[i] says where and whether the read is reverse-strand, desc[i] is the read's descriptor in the packed layout (word_off,
 * len, TPS_RD_HAS_INVALID exactly as the packers set it; tps::pack_layout of the lengths).  A read's codes take (len + 1) / 2 bytes,
 * rounded up to 16, from src[i].off on.  A device kernel expands the codes into seq2 / inv (reverse-strand reads reverse-complemented;
 * an IUPAC letter gets the code its ASCII gives, as in tps_batch_upload): the slot then holds an ordinary packed batch.  Pinned
 * sources are copied asynchronously, like tps_batch_upload_packed. */
int  tps_batch_upload_nib4(tps_ctx* ctx, int32_t slot, const uint8_t* nib, int64_t nib_bytes, const tps_nib_src* src,
                           const tps_read_desc* desc, int64_t n_reads, int64_t n_words);
/* Make `slot` of `ctx` refer to the resident packed batch of `src_slot` of ANOTHER context on the same device (no copy; the
 * batch stays owned by `src`, which must neither upload into that slot nor be destroyed while the borrower may still scan it;
 * `ctx`'s stream waits for `src`'s pending upload).  Several pattern tables over one batch -- `--telophrase 4 5 6`, the
 * reference's outer loop over k (Topsicle/main.py:206-235) -- are then scanned by one context per table at the same time:
 * every context keeps its own table, outputs and stream, the launches overlap on the GPU. */
int  tps_batch_share(tps_ctx* ctx, int32_t slot, tps_ctx* src, int32_t src_slot);
/* Pinned host memory for upload staging buffers (double buffering: fill one while the other is in flight). */
int  tps_host_alloc(tps_ctx* ctx, int64_t bytes, void** out);
int  tps_host_free(tps_ctx* ctx, void* p);
/* Download the resident packed batch of `slot` (tests: the device pack kernel vs the host packer; diagnostics).
 * seq2 / inv hold n_words entries, desc n_reads; any of the three may be NULL.  n_words out via *n_words_out. */
int  tps_batch_download_packed(tps_ctx* ctx, int32_t slot, uint32_t* seq2, uint16_t* inv, tps_read_desc* desc,
                               int64_t n_reads, int64_t n_words, int64_t* n_words_out);
/* Optional per-read tails (0/1) and pass flags for scans without TPS_F_STEP1. */
int  tps_batch_set_tails(tps_ctx* ctx, int32_t slot, const uint8_t* tails);

/* One pass of the hot path over a resident batch: patternTRC_count (allsteps.py:152-204) +
 * bound_detect's window loop (allsteps.py:257-297) + process_mean/Binseg
 * (allsteps.py:300-333), one 64-lane wave per read, one launch.  Asynchronous on the
 * context's stream; results land in context-owned pinned memory. */
int  tps_batch_scan(tps_ctx* ctx, int32_t slot, const tps_params* prm);
/* Wait for everything enqueued on the context's stream. */
int  tps_sync(tps_ctx* ctx);
/* Copy the per-read results of the last scan of `slot` (after tps_sync).  Every field of every read is written by every scan,
 * whether the read passes or not: a read that does not pass has n_win = 0, bkp = -1, gain = 0 and flags = 0. */
int  tps_batch_results(tps_ctx* ctx, int32_t slot, tps_read_result* out, int64_t n_reads);
/* Window layout of the last scan: win_off[n+1] (prefix of n_win over ALL reads of the batch,
 * scanned or not, computed from lengths and params only). */
int  tps_batch_window_offsets(tps_ctx* ctx, int32_t slot, int64_t* win_off, int64_t n_plus_1);
/* Reads that do not pass.  The window layout reserves the windows of EVERY read, and the scan kernels store S_w and c'_p only
 * for the reads that pass: `pass` = 1 in the last scan's results, decided by step 1 (TPS_F_STEP1: longer than min_len and the
 * better head count above min_count) or taken from tps_batch_set_tails (TPS_F_TAILS_IN: bit 1 set = skip).  For a read whose
 * `pass` is 0, tps_batch_window_sums, tps_batch_window_raw and tps_batch_read_sums return ZEROS for all of its windows, and
 * tps_batch_raw_to_fd writes zero rows for it (its CRC covers those zeros); tps_window_counts follows the same rule for the reads
 * its `tails` mark as skipped.  The library clears those ranges on the host after the copy (tps::clear_skipped_windows,
 * csrc/tps_plan.h), from the slot's own results: the scan launch itself clears nothing.  What these calls return therefore never
 * depends on what the device buffers held before. */
/* Download S_w (needs TPS_F_STORE_SUMS) / c'_p (needs TPS_F_STORE_RAW) of the last scan; zeros for the windows of reads that do
 * not pass (above). */
int  tps_batch_window_sums(tps_ctx* ctx, int32_t slot, int32_t* sums, int64_t n_windows);
int  tps_batch_window_raw(tps_ctx* ctx, int32_t slot, uint8_t* raw, int64_t n_windows_times_p);
/* c'_p of SELECTED reads of the last scan (needs TPS_F_STORE_RAW) straight to a file (ABI 4): the rows of reads[0 .. n_sel)
 * -- ascending indices into the batch -- back to back, u8[n_win x P] each, at byte `file_off` of `fd` (pwrite: the descriptor's
 * own position is not used, several contexts may write into one file at once).  The rows never stop in the caller's memory:
 * device -> two pinned pieces of the context -> pwritev, the next piece copied while the current one is written.  crc_fn (may be
 * NULL; e.g. libtopsicle_io.so's tps_crc32) is run over the bytes in file order, starting from 0: *crc_out (may be NULL) is the
 * CRC-32 of exactly what was written, *bytes_out its length -- a caller that lays the blocks of many batches into one zip / npy
 * member joins the per-block values with crc32_combine.  Replaces, for the columnar raw-count output, the per-read
 * DataFrame.to_csv of the reference (Topsicle/main.py:146-150; Topsicle/allsteps.py:398-411 builds the rows).  A selected read
 * that does not pass gets n_win x P zero bytes ("Reads that do not pass" above), and the CRC covers them. */
typedef uint32_t (*tps_crc32_fn)(uint32_t crc, const uint8_t* p, int64_t n);
int  tps_batch_raw_to_fd(tps_ctx* ctx, int32_t slot, const int64_t* reads, int64_t n_sel, int fd, int64_t file_off,
                         tps_crc32_fn crc_fn, uint32_t* crc_out, int64_t* bytes_out);
/* S_w of ONE read of the last scan (any scan with TPS_F_WINDOWS; n_windows = the read's windows in the layout); zeros for a read
 * that does not pass ("Reads that do not pass" above). */
int  tps_batch_read_sums(tps_ctx* ctx, int32_t slot, int64_t read, int32_t* sums, int64_t n_windows);
/* Step-1 per-pattern counts of the last scan: c_start[n*P], c_end[n*P] (int32).  Every count of every read is written by every
 * scan that runs step 1, whether the read passes or not (a read shorter than k letters counts zero everywhere). */
int  tps_batch_trc_counts(tps_ctx* ctx, int32_t slot, int32_t* c_start, int32_t* c_end, int64_t n_reads);

/* ---- one-shot host-pointer calls (parity tests, per-read API) -------------------------- */
/* patternTRC_count's counting loop (allsteps.py:176-184): integer counts only; the float64
 * TRC, arg-max and cutoff stay in the host language so they are bit-identical. */
int  tps_trc_counts(tps_ctx* ctx, const uint8_t* bases, const int64_t* offsets, int64_t n_reads,
                    int32_t no_bp, int32_t* c_start, int32_t* c_end);
/* bound_detect / rawCountPattern window loops (allsteps.py:275-291, 398-411) for the given
 * tail per read.  win_off[n+1] must be the prefix of tps_window_count() over the reads.
 * sums: int32[win_off[n]]; raw: u8[win_off[n]*P] or NULL.  tails[i]: bit 0 = the tail, bit 1 = skip the read -- the windows of
 * a skipped read come back as zeros in sums and raw ("Reads that do not pass" above). */
int  tps_window_counts(tps_ctx* ctx, const uint8_t* bases, const int64_t* offsets,
                       const uint8_t* tails, int64_t n_reads, int32_t window, int32_t slide,
                       int32_t trimfirst, int32_t maxlen, const int64_t* win_off,
                       int32_t* sums, uint8_t* raw);
/* rpt.Binseg(model="l2").fit(y).predict(n_bkps=1) (allsteps.py:310-311) on integer window
 * sums: bkp[n] (-1 = no admissible split), gain[n] (may be NULL). */
int  tps_binseg_l2(tps_ctx* ctx, const int32_t* sums, const int64_t* win_off, int64_t n_reads,
                   int32_t n_patterns, int32_t jump, int32_t min_size, int32_t* bkp, double* gain);
/* The same, also reporting per read whether the exact tournament decided (tie[n]: 1 = TPS_RES_TIE, see above; may be NULL). */
int  tps_binseg_l2_ties(tps_ctx* ctx, const int32_t* sums, const int64_t* win_off, int64_t n_reads,
                        int32_t n_patterns, int32_t jump, int32_t min_size, int32_t* bkp, double* gain, uint8_t* tie);

/* Number of windows seq_cut_windows yields for a read of length L (allsteps.py:219, 263-271). */
int64_t tps_window_count(int64_t read_len, int32_t window, int32_t slide, int32_t trimfirst, int32_t maxlen);

/* ---- exploratory counts (overview plots) ------------------------------------------------- */
/* patterns_vs_match_heatmap's counting loop (descriptive_plot.py:259-291): for every read of the resident batch longer
 * than min_len, in bases [lo, hi) of the read (strand 0) and of its reverse complement (strand 1), the leftmost
 * non-overlapping matches of  kmer(.{follow})  for each of the first n_fwd patterns of the table -- the k-mers of the
 * doubled motif; the table must hold their complements behind them, as patterns_to_search builds it (allsteps.py:104-120).
 *   picks  uint32[n_reads][2][n_fwd][pw], pw = ceil((hi - lo) / 32): bit j of word w = a match starts at base lo + 32 w + j
 *          of that strand's string (the reference's DataFrame rows: Pattern = the k-mer, Match = the `follow` letters
 *          behind it, which the caller reads from its own copy of the read)
 *   hist   int64[2][n_fwd][4^follow + 1] or NULL: the crosstab summed over the batch; the bin of a match is the 2-bit
 *          code of the following bases (first base in the low bits, A C T G = 0 1 2 3, as the reference's upper-cased,
 *          complemented strand-1 string spells them); the last bin counts matches followed by a non-ACGT letter.
 * follow <= 8, hi - lo <= 4096, n_fwd <= 15. */
int  tps_batch_kmer_followers(tps_ctx* ctx, int32_t slot, int32_t n_fwd, int32_t follow, int32_t lo, int32_t hi,
                              int32_t min_len, uint32_t* picks, int64_t picks_words, int64_t* hist, int64_t hist_len);
/* The same on the table of tps_set_patterns_wide (which takes narrow tables too; a table set with tps_set_patterns is
 * TPS_E_PATTERN here): k <= TPS_WIDE_MAX_K, 1 <= n_fwd <= 32 with 2 n_fwd <= n_patterns, follow >= 0, hi - lo <= 4096 -- the
 * doubled form of every motif of up to 32 letters at every k, however many letters follow the k-mer.  picks and hist are laid
 * out as above and, on a table both calls accept, bit-identical.  hist has 4^follow + 1 bins: it may be non-NULL for
 * follow <= 8 only (TPS_E_CAPACITY otherwise); for more following letters the caller counts the rows it builds from picks.
 * One launch of tps_followers_kernel_wide. */
int  tps_batch_kmer_followers_wide(tps_ctx* ctx, int32_t slot, int32_t n_fwd, int32_t follow, int32_t lo, int32_t hi,
                                   int32_t min_len, uint32_t* picks, int64_t picks_words, int64_t* hist, int64_t hist_len);

/* ---- motif census (finding the motif from the reads) ------------------------------------- */
/* What repeats at the ends of the reads, without a pattern table (tps_set_patterns need not have been called; the reference
 * leaves this to other tools: its README names Tandem Repeats Finder and tidk).  For every read of the resident batch longer
 * than min_len and each end e, let h = bases [lo, min(L, hi)) of the upper-cased read (e = 0) or of its reverse complement
 * (e = 1) -- both "telomere first", as step 1 looks at them -- and n = len(h).  For a period u in [u_min, u_max], w = min(u, 8):
 *   eq_u[i]  = 1 iff i + u < n and h[i], h[i + u] are both one of ACGT and equal
 *   per_u[i] = 1 iff i + u + w <= n and eq_u[i .. i + w - 1] are all 1        (the w-mer at i recurs u bases on)
 *   C_u      = sum over i of per_u[i]
 * u* is the period with the largest C_u (ties: the smallest u); the run is the longest maximal run of consecutive i with
 * per_u*[i] = 1 (ties: the leftmost).  w stops at 8 so that a long motif keeps its support at nanopore error rates.
 *   hits   tps_motif_hit[n_reads][2]: period = u*, support = C_u*, run_start / run_len = the run, n_bases = n, unit = the u*
 *          letters h[run_start .. run_start + u*) as 2-bit codes (A C T G = 0 1 2 3, letter j in bits [2j, 2j+1]; a letter
 *          of the unit that is not ACGT -- possible behind its first 8 -- has the code (ASCII >> 1) & 3 of the packed batch,
 *          complemented at e = 1).  All zeros where no C_u is positive, and for reads of min_len bases or fewer.
 *   counts int32[n_reads][2][u_max - u_min + 1] or NULL: every C_u.
 * 1 <= u_min <= u_max <= 32 (TPS_E_ARG), hi - lo <= 4096 (TPS_E_CAPACITY).  What a caller makes of the hits (a floor on the
 * support, the vote over the read ends) is its own: topsicle_amd.motif.  One launch; returns when the outputs are in place. */
typedef struct tps_motif_hit {        /* 32 bytes */
    uint64_t unit;
    int32_t period;
    int32_t support;
    int32_t run_start;
    int32_t run_len;
    int32_t n_bases;
    int32_t reserved;
} tps_motif_hit;
int  tps_batch_motif_census(tps_ctx* ctx, int32_t slot, int32_t u_min, int32_t u_max, int32_t lo, int32_t hi, int32_t min_len,
                            tps_motif_hit* hits, int64_t n_hits, int32_t* counts, int64_t counts_len);

/* ---- variant census (what the called telomere tract is made of) ---------------------------- */
/* Canonical repeats, units with one substituted letter, and the rest, for a tract [begin, end) per read of the resident batch;
 * no pattern table (the reference has nothing comparable).  `unit` is a primitive word U of m letters, 2 <= m <= 32, as
 * tps_motif_hit.unit spells it: 2-bit codes A C T G = 0 1 2 3, letter j in bits [2j, 2j+1], nothing behind them; not a power of
 * a shorter word.  For read r, h = the upper-cased read (tails[r] = 0) or its reverse complement (tails[r] = 1) -- "telomere
 * first", the orientation the motif census uses and --pattern is given in -- and end[r] is clamped to L.  A read with
 * end - begin < m contributes nothing (its row stays zero).  Otherwise every i in [begin, end - m] is EXAMINED (n += 1), with
 * x = h[i .. i + m) and R_j = U rotated left by j (R_j[q] = U[(j + q) mod m]):
 *   - a letter of x that is not ACGT: the position is "other";
 *   - else the smallest j with Hamming(x, R_j) <= 1 decides: distance 0 is CANONICAL; distance 1 with the mismatch at q is the
 *     VARIANT (p, c), p = (j + q) mod m the place in U as given, c the code of the letter x[q]  (U = AAAC, x = AAAA: j = 0,
 *     p = 3, c = A).  The rotations of a primitive word differ pairwise in >= 2 places: a canonical position is never a variant;
 *   - no such j: "other".
 * The position falls in bin min((end - 1 - i) / bin, n_bins - 1): bins are measured back from the boundary.
 *   counts  uint32[n_reads][2 + 4m]: [0] = n, [1] = canonical, [2 + 4p + c] = variant (p, c) (c = U[p] stays 0);
 *           other = n - everything else.
 *   profile int64[n_bins][2 + 4m] or NULL: the same row summed over all reads of the batch, per bin.
 * Both are exact sums: identical from run to run.  TPS_E_ARG: m outside 2..32, a unit that is a power of a shorter word (or has
 * codes behind its m letters), a negative begin / end, begin > end, a tail other than 0 / 1, n_reads or an array length that
 * does not match the slot.  TPS_E_CAPACITY: bin outside 64..4064, n_bins outside 1..64.  TPS_E_STATE: an empty slot.
 * One launch; returns when the outputs are in place.  The slot's scan state (tails, results, sums, raw rows) is not touched. */
int  tps_batch_variant_census(tps_ctx* ctx, int32_t slot, uint64_t unit, int32_t m, const uint8_t* tails, const int32_t* begin,
                              const int32_t* end, int64_t n_reads, int32_t bin, int32_t n_bins, uint32_t* counts,
                              int64_t counts_len, int64_t* profile, int64_t profile_len);

/* ---- tract map (telomere-repeat tracts anywhere in a read, on either strand) ---------------- */
/* Where in the WHOLE read repeats of a unit lie; no pattern table, nothing assumed about the read's ends (the reference has
 * nothing comparable).  `unit` is a primitive word U of m letters, 4 <= m <= 32, spelled as tps_motif_hit.unit and
 * tps_batch_variant_census spell it.  Strand 0 is U as given (the C strand, what a read's head shows), strand 1 its reverse
 * complement; the read is always taken forward, as stored, upper-cased.
 *   word    w = min(m, 8).  The cyclic words of a unit V are the m words (V V ...)[j .. j + w), j = 0 .. m - 1.
 *   hit     position i in [0, L - w] is a hit on strand s when read[i .. i + w) has only ACGT letters and differs in at most one
 *           place from some cyclic word of U_s.
 *   block   block j holds the positions [j block, (j + 1) block) of [0, L - w]: nb = ceil((L - w + 1) / block) blocks, none
 *           when L < w.  count_s[j] = its hits; it is FLAGGED when count_s[j] >= min_hits (a short last block: same threshold).
 *   tract   on strand s, a maximal run of flagged blocks j_0 < ... < j_t with j_(i+1) - j_i <= gap + 1 (at most `gap` unflagged
 *           blocks between neighbours); b = j_0, e = j_t + 1; kept when e - b >= min_blocks.  begin = b block,
 *           end = min(e block + w - 1, L), blocks = e - b, hits = the sum of count_s over [b, e), inner gaps included.
 *           Unflagged blocks at either side never belong to a tract.
 *   found   int32[n_reads][2]: the true number of kept tracts of strand s.
 *   tracts  tps_tract[n_reads][2][max_tracts]: the first max_tracts of them in order of begin, the rest of the row zero.
 *   totals  uint32[n_reads][4]: hits of strand 0, of strand 1, flagged blocks of strand 0, of strand 1, over the whole read.
 * Exact integers, identical from run to run.  TPS_E_ARG: m outside 4..32, a unit that is a power of a shorter word (or has codes
 * behind its m letters), an array length that does not match the slot.  TPS_E_CAPACITY: block no multiple of 64 in 64..1024,
 * min_hits outside 1..block, gap outside 0..64, min_blocks outside 1..64, max_tracts outside 1..16.  TPS_E_STATE: an empty slot.
 * One launch; returns when the outputs are in place.  The slot's scan state (tails, results, sums, raw rows) is not touched. */
typedef struct tps_tract {            /* 16 bytes */
    int32_t begin, end;               /* bases [begin, end) of the read as stored */
    int32_t hits, blocks;
} tps_tract;
int  tps_batch_tract_map(tps_ctx* ctx, int32_t slot, uint64_t unit, int32_t m, int32_t block, int32_t min_hits, int32_t gap,
                         int32_t min_blocks, int32_t max_tracts, tps_tract* tracts, int64_t tracts_len, int32_t* found,
                         int64_t found_len, uint32_t* totals, int64_t totals_len);

/* ---- end groups (which chromosome end a telomeric read came from) --------------------------- */
/* A sketch of the subtelomere behind the called boundary of every read of the resident batch, and the links between sketches
 * that share enough of it; no pattern table (the reference has nothing comparable).  `unit`, m: a primitive word of 4 <= m <= 32
 * letters, spelled as tps_batch_tract_map takes it.  For read r, h = the upper-cased read (tails[r] = 0) or its reverse
 * complement (tails[r] = 1) -- "telomere first", as in tps_batch_variant_census -- and end[r] is clamped to L.
 *   word    w = min(m, 8).  h[p .. p + w) is a REPEAT WORD when it has only ACGT letters and differs in at most one place from a
 *           cyclic word of the unit or of its reverse complement (a hit on either strand of the tract map's rule).
 *   kept    the k-mer at i in [begin, end - k] is KEPT when its k letters are all ACGT and none of its k - w + 1 words
 *           h[i + d .. i + d + w), d = 0 .. k - w, is a repeat word: telomere k-mers, and their one-error variants, are the
 *           same in every read and say nothing about the end.
 *   hash    c = sum of code(h[i + q]) << 2q over q < k (A C T G = 0 1 2 3) as a uint32; x = fmix32(c ^ 0x9E3779B9), fmix32 =
 *           MurmurHash3's 32-bit finaliser (x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16, modulo
 *           2^32); bucket = x >> (32 - log2 buckets).
 *   sketch  uint32[n_reads][buckets]: the smallest hash of each bucket, 0xFFFFFFFF for an empty one (a hash that equals
 *           0xFFFFFFFF counts as empty).  A read with end - begin < k has an empty row.
 *   kept    uint32[n_reads]: the number of kept k-mers.
 * Exact, identical from run to run (a minimum does not depend on order).  TPS_E_ARG: m outside 4..32, a unit that is a power of
 * a shorter word (or has codes behind its m letters), buckets not 64 / 128 / 256 / 512, a negative begin / end, begin > end, a
 * tail other than 0 / 1, n_reads or an array length that does not match the slot.  TPS_E_CAPACITY: k outside 8..16,
 * end - begin > 16384.  TPS_E_STATE: an empty slot.  One launch; returns when the outputs are in place.  The slot's scan state
 * (tails, results, sums, raw rows) is not touched. */
int  tps_batch_end_sketch(tps_ctx* ctx, int32_t slot, uint64_t unit, int32_t m, int32_t k, int32_t buckets, const uint8_t* tails,
                          const int32_t* begin, const int32_t* end, int64_t n_reads, uint32_t* sketch, int64_t sketch_len,
                          uint32_t* kept, int64_t kept_len);
/* All pairs of n sketches (rows of `sketch`, uint32[n][buckets], from the host; no resident batch needed).  match(i, j) = the
 * number of buckets b with s_i[b] == s_j[b], both not 0xFFFFFFFF.  For every row i:
 *   degree  int32[n]: the true number of j > i with match(i, j) >= min_match.
 *   links   int32[n][max_links]: the smallest such j in ascending order, the rest of the row -1.
 *   matches int32[n][max_links]: match(i, j) beside each link, the rest of the row 0.
 * Exact, identical from run to run.  TPS_E_ARG: buckets not 64 / 128 / 256 / 512, an array length that does not match n.
 * TPS_E_CAPACITY: n over 262144, min_match outside 1..buckets, max_links outside 1..256.  One launch; returns when the outputs
 * are in place. */
int  tps_sketch_links(tps_ctx* ctx, const uint32_t* sketch, int64_t n, int32_t buckets, int64_t sketch_len, int32_t min_match,
                      int32_t max_links, int32_t* degree, int64_t degree_len, int32_t* links, int64_t links_len, int32_t* matches,
                      int64_t matches_len);

/* ---- anchored lengths (one boundary per end group, in the coordinates of one of its reads) --- */
/* The KEPT WINDOW of every read of the resident batch: what tps_batch_end_sketch hashes, handed out position by position.  The
 * same telomere-first string h, the same window [begin, min(end, L)), the same unit, k and KEPT rule; span = the longest window,
 * k <= span <= 4096.  Rows of (span + 15) / 16 and (span + 31) / 32 dwords, every dword written:
 *   codes   letter q of the window (h[begin + q]) as a 2-bit code (A C T G = 0 1 2 3, already complemented for tail 1) at bits
 *           2 (q & 15) of dword q >> 4; a letter that is not ACGT, and everything behind the window's last letter, is 0.
 *   keep    bit q & 31 of dword q >> 5 is set exactly when the k-mer at begin + q is KEPT; popcount(keep[r]) == kept[r] of the
 *           sketch of the same window.
 * Exact, identical from run to run.  The checks and codes of tps_batch_end_sketch (TPS_E_ARG: the unit, a tail other than 0 / 1, a
 * negative begin / end, begin > end; TPS_E_CAPACITY: k outside 8..16, end - begin > 16384; TPS_E_STATE: an empty slot), and
 * TPS_E_CAPACITY: span outside k..4096, end - begin > span; TPS_E_ARG: n_reads or an array length that does not match the slot and
 * span.  One launch; returns when the outputs are in place.  The slot's scan state is not touched. */
int  tps_batch_end_window(tps_ctx* ctx, int32_t slot, uint64_t unit, int32_t m, int32_t k, const uint8_t* tails, const int32_t* begin,
                          const int32_t* end, int64_t n_reads, int32_t span, uint32_t* codes, int64_t codes_len, uint32_t* keep,
                          int64_t keep_len);
/* The offset of window i against window ref[i], for n windows from the host (rows as tps_batch_end_window writes them, length[i]
 * letters each; no resident batch needed).  The kept positions of a window are the p in [0, length - k] whose keep bit is set;
 * x(p) = fmix32(c ^ 0x9E3779B9) of the k-mer's codes c, as in the sketch (fmix32 is a bijection: equal x, equal k-mer).
 *   table   of the reference R: 4096 slots, empty = 0xFFFFFFFF; every kept q of R does
 *           T[x >> 20] = min(T[x >> 20], ((x & 0xFFFFF) << 12) | q): the smallest low 20 bits win a slot, then the smallest q.
 *   votes   a kept p of the query Q with t = T[x >> 20], t != empty and (t >> 12) == (x & 0xFFFFF), votes for the diagonal
 *           d = (t & 4095) - p, -4096 < d < 4096.
 *   coarse  H[(d + 4096) >> 6]++ over 128 bins; pair[c] = H[c] + H[c + 1], c = 0 .. 126; best = the smallest c with the largest
 *           pair; second = the largest pair[c] with |c - best| >= 2, 0 if there is none.
 *   fine    the 128 diagonals 64 best - 4096 <= d < 64 best - 3968: votes = their number (= pair[best]); offset = their lower
 *           median, element (votes - 1) / 2 of the sorted votes, 0 when votes == 0.
 * offset, votes, second: int32[n], in window coordinates (the caller adds begin_R - begin_Q).  A row with ref[i] < 0 gets 0, 0, 0;
 * ref[i] == i is allowed.  Exact, identical from run to run (minima and counts do not depend on order).  TPS_E_CAPACITY: n over
 * 262144, span outside k..4096, k outside 8..16.  TPS_E_ARG: ref[i] >= n, length[i] outside 0..span, out_len != n.  One launch;
 * returns when the outputs are in place. */
int  tps_window_offsets(tps_ctx* ctx, const uint32_t* codes, const uint32_t* keep, const int32_t* length, const int32_t* ref, int64_t n,
                        int32_t span, int32_t k, int32_t* offset, int32_t* votes, int32_t* second, int64_t out_len);

/* ---- named ends (end groups placed on the ends of a reference) ------------------------- */
/* n query windows placed on n_ref reference windows, all from the host (no resident batch and no pattern table needed).  Both sets
 * are rows as tps_batch_end_window writes them -- codes, keep, length[i] letters -- with one span and one k; kept positions and
 * x(p) = fmix32(c ^ 0x9E3779B9) are those of tps_window_offsets.
 *   index    an ENTRY is (x, r, q) for every kept q of every reference row r.  A k-mer with more than max_occ entries over ALL
 *            reference rows is dropped whole; every other entry takes part (no slot is fought over: no k-mer is lost to another,
 *            and a k-mer several rows share counts for each of them, once per entry).
 *   matches  of query i: every (r, q, p) with p kept in the query and (x(p), r, q) an entry.
 *   total    total[r] = the matches on row r.  ref = the smallest r with the largest total, -1 where the query has no match.
 *            runner_ref = the smallest r != ref with the largest total among the other rows, -1 where no other row has a match;
 *            runner = that row's total, or 0.
 *   coarse   over the matches of row ref only, d = q - p: H[(d + 4096) >> 6]++ over 128 bins; pair, best and second exactly as in
 *            tps_window_offsets.
 *   fine     the 128 diagonals of the best pair: votes = their number (= pair[best]), offset = their lower median.
 * ref, total (of row ref), runner_ref, runner, offset, votes, second: int32[n] each, every entry written, offset in window
 * coordinates.  A query with length < k or without a match gets -1, 0, -1, 0, 0, 0, 0.  A reference row with length < k or no keep
 * bit has no entry.  Exact, identical from run to run (minima and counts do not depend on order).  TPS_E_CAPACITY: n over 262144,
 * n_ref outside 1..1024, span outside k..4096, k outside 8..16, max_occ outside 1..64.  TPS_E_ARG: codes_len / keep_len /
 * ref_codes_len / ref_keep_len that are not n resp. n_ref rows of (span + 15) / 16 resp. (span + 31) / 32 dwords, out_len != n, a
 * length or ref_length outside 0..span.  The index is built on the host once per call (sorted entries behind a directory over
 * the top bits of x; 16 bytes per entry, at most n_ref x 4096 entries = 64 MB); one launch; returns when the outputs are in place. */
int  tps_window_place(tps_ctx* ctx, const uint32_t* codes, int64_t codes_len, const uint32_t* keep, int64_t keep_len, const int32_t* length,
                      int64_t n, const uint32_t* ref_codes, int64_t ref_codes_len, const uint32_t* ref_keep, int64_t ref_keep_len,
                      const int32_t* ref_length, int32_t n_ref, int32_t span, int32_t k, int32_t max_occ, int32_t* ref, int32_t* total,
                      int32_t* runner_ref, int32_t* runner, int32_t* offset, int32_t* votes, int32_t* second, int64_t out_len);

/* ---- windows aligned base by base (what a consensus of an end group is called from) ---------------------------------------- */
/* n query windows, each aligned against one of n_ref reference windows inside a band of 64 diagonals, all from the host (no resident
 * batch and no pattern table needed).  Both sets are codes rows as tps_batch_end_window writes them, (span + 15) / 16 dwords each
 * with one span, length[i] resp. ref_length[r] letters; keep bits and k play no part.  A letter that is not ACGT arrives as code 0
 * and is read as A.  ref[i] = the reference row of query i (< 0: none), centre[i] = the diagonal c the band sits on, with the
 * meaning of tps_window_offsets' offset: reference position = query position + c.
 *   band      Q = the query, n letters; R = its reference row, m letters.  Lane l, 0 <= l < 64, owns the diagonal d = c - 32 + l.
 *             The band is the set of cells (i, j) with 0 <= i <= n, 0 <= j <= m and j - i = d for some lane; every cell outside
 *             it is infinite.
 *   start     D(i, j) = 0 on the band cells with i = 0 or j = 0: both leading ends are free.
 *   step      D(i, j) = min(D(i-1, j-1) + [Q[i-1] != R[j-1]],  D(i-1, j) + 1 (lane l + 1 of the row before),
 *             D(i, j-1) + 1 (lane l - 1 of the same row)).
 *   end       among the band cells with i = n or j = m the smallest D; ties go to the largest i, then to the largest j.  dist = that
 *             D.  No such finite cell (the band misses the matrix), or ref[i] < 0: flag NONE, every number 0, every column "not
 *             covered".
 *   path      from the end cell while i > 0 and j > 0, the first that holds: diagonal if D(i, j) = D(i-1, j-1) + s, s = 0 or 1 --
 *             column j-1 carries the letter Q[i-1]; else up if D(i, j) = D(i-1, j) + 1 -- Q[i-1] is an inserted letter; else left --
 *             column j-1 is deleted.  (q_begin, r_begin) = the cell where it stops, (q_end, r_end) = the end cell; the columns
 *             r_begin <= j < r_end are covered.
 *   inserted  letters are recorded on the column j they stand in front of, and only where r_begin < j < r_end: those in front of
 *             the first covered column or behind the last are recorded nowhere.
 *   EDGE      set when a cell the path stands on with i > 0 and j > 0 lies on lane 0 or lane 63.
 * Outputs, every entry written:
 *   stat      int32[n][6]: dist, q_begin, q_end, r_begin, r_end, flags (bit 0 NONE, bit 1 EDGE).
 *   cols      uint16[n][span], or NULL (not asked for): bits 0-2 the state -- 0..3 the query's letter on that column, 4 deleted,
 *             7 not covered; bits 3-4 min(inserted letters in front of the column, 3); bits 5-6 the first inserted letter; bits
 *             7-8 the second; everything 0 where it does not apply.
 *   pile      int32[n_pile][span][13], or NULL, with pile_row int32[n]: cleared by the call; a pair with pile_row[i] >= 0 and neither
 *             flag set adds, per covered column, one count to its state (A C T G del = entries 0..4), per recorded insertion one
 *             to ins1[first letter] (entries 5..8) and, with two or more inserted letters, one to ins2[second letter] (entries
 *             9..12).
 * Exact, identical from run to run (integer sums do not depend on order).  ref[i] pointing at a row equal to the query is an
 * ordinary pair with dist 0.  TPS_E_CAPACITY: n over 262144, n_ref outside 1..262144, span outside 1..4096, n_pile outside 0..n_ref.
 * TPS_E_ARG: codes_len / ref_codes_len / stat_len / cols_len / pile_len that do not match (0 for a piece that is NULL), pile with
 * n_pile = 0, n_pile > 0 without pile_row, a length or ref_length outside 0..span, ref[i] >= n_ref, |centre[i]| > 4096,
 * pile_row[i] >= n_pile.  One launch (one wave per pair, one lane per diagonal; dynamic LDS sized by span and by the longest query);
 * returns when the outputs are in place. */
int  tps_window_align(tps_ctx* ctx, const uint32_t* codes, int64_t codes_len, const int32_t* length, int64_t n, const uint32_t* ref_codes,
                      int64_t ref_codes_len, const int32_t* ref_length, int32_t n_ref, const int32_t* ref, const int32_t* centre,
                      int32_t span, int32_t* stat, int64_t stat_len, uint16_t* cols, int64_t cols_len, const int32_t* pile_row,
                      int32_t* pile, int32_t n_pile, int64_t pile_len);

/* ---- adapters at the telomere end (which reads start at the real chromosome end, and with which barcode) ---- */
/* Up to 64 given sequences searched approximately in a region of every read of the resident batch; no pattern table (the
 * reference has nothing comparable).  For read r, h = the upper-cased read (tails[r] = 0) or its reverse complement
 * (tails[r] = 1) -- "telomere first", as in tps_batch_variant_census.
 *   region   T = h[begin[r] .. min(end[r], L)), n = |T|, 0 <= n <= 1024 (begin at or past the read's end: n = 0).
 *   patterns pattern j = A_j, m_j = pat_len[j] letters of ACGT, 12 <= m_j <= 64, 0 <= j < n_pat, 1 <= n_pat <= 64, in the
 *            orientation of h: a sequence expected at the 3' end of tail-1 reads is given reverse-complemented; the same list is
 *            searched on both tails.  2-bit codes A C T G = 0 1 2 3, letter i in bits [2i, 2i + 1] of the 128 bits of
 *            patterns[2j] (letters 0 .. 31) and patterns[2j + 1] (letters 32 .. 63), nothing behind the m_j letters.
 *   distance D_j(e), e = 0 .. n: the smallest unit-cost edit distance (substitution, insertion, deletion: 1 each) between A_j and
 *            any substring T[s .. e), 0 <= s <= e -- Sellers' recurrence D[0][e] = 0, D[i][0] = i,
 *            D[i][e] = min(D[i-1][e-1] + (A_j[i-1] != T[e-1]), D[i-1][e] + 1, D[i][e-1] + 1), D_j(e) = D[m_j][e].  A letter of T that
 *            is not ACGT matches nothing.  D_j(0) = m_j.
 *   hits     uint16[n_reads][n_pat][2] = (dist_j, end_j): dist_j = the minimum of D_j(e) over e, end_j = the smallest e that
 *            reaches it, relative to begin[r]; an empty region gives (m_j, 0).  Every entry is written.
 * Exact, identical from run to run; the answer depends on nothing outside the region.  TPS_E_CAPACITY: n_pat outside 1..64, a
 * pat_len outside 12..64, end - begin > 1024.  TPS_E_ARG: codes behind a pattern's letters, a tail other than 0 / 1, a negative
 * begin / end, begin > end, n_reads or hits_len that does not match the slot and n_pat.  TPS_E_STATE: an empty slot.  One launch
 * (one wave per read, one lane per pattern, Myers' bit-vector recurrence); returns when the outputs are in place.  The slot's scan
 * state (tails, results, sums, raw rows) is not touched. */
int  tps_batch_adapter_find(tps_ctx* ctx, int32_t slot, const uint64_t* patterns, const int32_t* pat_len, int32_t n_pat,
                            const uint8_t* tails, const int32_t* begin, const int32_t* end, int64_t n_reads, uint16_t* hits,
                            int64_t hits_len);

/* ---- the boundary at base resolution, and its support -------------------------------------------------------------------- */
/* One change point per read on the per-position hits of the telomere repeat, by likelihood, with the evidence for it; no pattern
 * table (the reference has nothing comparable).  unit, m: as tps_batch_tract_map takes them, 4 <= m <= 32, a primitive word;
 * w = min(m, 8).  For read r, h = the telomere-first string of tps_batch_variant_census: the upper-cased read (tails[r] = 0) or its
 * reverse complement (tails[r] = 1).  end[r] is clamped to L.  N = end - begin - w + 1 positions (N <= 0: none).
 *   hit      for i in [begin, begin + N): x_i = 1 when h[i .. i + w) has only ACGT letters and is within Hamming distance 1 of a
 *            cyclic word of U; else 0.  This is strand 0 of the tract map's rule applied to h; for tail 1 it is the read's strand-1
 *            hit at the mirrored position.
 *   score    s_i = x_i ? +hit : -miss.  P(begin) = 0, P(j) = the sum of s_i over begin <= i < j, for j in [begin, begin + N]: the
 *            log-likelihood of "telomere up to j, not telomere from j on", up to a constant.  A stretch keeps extending the tract
 *            while its hit density exceeds miss / (hit + miss).
 *   pos      the smallest j with P(j) maximal; score = P(pos).  pos = begin when nothing scores positive.
 *   drop     score - P(begin + N), always >= 0; 0 when the tract runs to the region's end.
 *   at_score P(clamp(at[r], begin, begin + N)): the caller passes the boundary it has called there.
 *   hits     hits_before = the sum of x_i over i < pos; hits_after = the rest.
 *   runner   the maximum of P(j) over the j with |j - pos| >= sep; runner_pos = the smallest such j.  Where there is no such j:
 *            runner = 0, runner_pos = -1.  score - runner says how much worse the best boundary at least sep away is.
 *   empty    a read with N <= 0 gets pos = begin, runner_pos = -1, everything else 0.
 * Every row is written whole, every time; exact integers, identical from run to run.  TPS_E_ARG: the unit rules of
 * tps_batch_tract_map, a negative begin / end / at, begin > end, a tail other than 0 / 1, n_reads or out_len that does not match
 * the slot, null arrays with reads in the slot.  TPS_E_CAPACITY: hit or miss outside 1..16, sep outside 1..65535,
 * end - begin > 65536 after end is clamped to L (named with the read: "read 7: ...").  TPS_E_STATE: an empty slot.  An empty batch
 * is TPS_OK.  One launch (one wave per read); returns when the rows are in place.  The slot's scan state (tails, results, sums, raw
 * rows) is not touched. */
typedef struct tps_refine { int32_t pos, score, drop, at_score, hits_before, hits_after, runner, runner_pos; } tps_refine; /* 32 bytes */
int  tps_batch_boundary_refine(tps_ctx* ctx, int32_t slot, uint64_t unit, int32_t m, const uint8_t* tails, const int32_t* begin,
                               const int32_t* end, const int32_t* at, int64_t n_reads, int32_t hit, int32_t miss, int32_t sep,
                               tps_refine* out, int64_t out_len);

/* ---- base modifications against the boundary ------------------------------------------------------------------------------- */
/* The calls of one base modification (BAM MM / ML tags, as tps_bam_mods_spans of include/topsicle_io.h lists them: skip counts among
 * the read's C's and probability bytes) put on the resident read and binned against a boundary; no pattern table (the reference has
 * nothing comparable).  Read r owns the entries mod_off[r] .. mod_off[r + 1] of delta[] / prob[].  end[r] is clamped to L; the
 * region [begin, end) is in the coordinates of the telomere-first string, t = p (tails[r] = 0) or L - 1 - p (1) for the position p
 * of the resident read -- the read as sequenced, which is what MM counts along.
 *   C, CpG   p is a C when its base is c or C; a CpG when also p + 1 < L and the base there is g or G.  Read orientation, whatever
 *            the tail.
 *   ordinal  entry j has o_j = (delta_0 + 1) + ... + (delta_j + 1) - 1, carried in 64 bits, saturating: it never wraps.
 *   landing  o_j >= c_total, the read's C's: `beyond`; one such entry sets TPS_MOD_BAD in flags and makes every bin of the read,
 *            and cpg and called of its row, zero.  Otherwise the entry sits on the o_j-th C (from 0) at p, and is in_region when
 *            begin <= t < end; in the region and not on a CpG: off_context; else it falls into bin floor((t - origin) / w) + nb0.
 *   bins     nb0 bins of w bases in front of origin, nb1 behind: called = the entries, sum = the sum of their prob bytes, high =
 *            those with prob >= hi, low = those with prob <= lo; cpg = the CpGs of the sequence whose t falls into the bin,
 *            whatever the tags say.
 *   row      c_total, entries (mod_off[r + 1] - mod_off[r]), beyond, in_region, off_context, cpg and called summed over the bins,
 *            flags.
 *   empty    a read with begin >= end after the clamp gets a row and bins of zeros.
 * Every row and every bin record is written whole, every time; exact integers, identical from run to run.  TPS_E_CAPACITY: w outside
 * 16..4096, nb0 + nb1 outside 1..64, end - begin > 16384 after the clamp (named with the read: "read 7: ...").  TPS_E_ARG: lo < hi
 * within 0..255 does not hold, a negative begin / end / origin, begin > end, a tail other than 0 / 1, a region that is not empty and
 * leaves [origin - nb0 w, origin + nb1 w), n_reads / rows_len / bins_len that do not match the slot, mod_off that does not ascend
 * from a value >= 0 to n_mods, null arrays with reads in the slot.  TPS_E_STATE: an empty slot.  An empty batch is TPS_OK.  One launch
 * (one wave per read); returns when rows and bins are in place.  The slot's scan state is not touched. */
#define TPS_MOD_BAD 1u          /* tps_mod_row.flags: an entry lies beyond the read's last C (a tag that does not belong to these bases) */
typedef struct tps_mod_row { uint32_t c_total, entries, beyond, in_region, off_context, cpg, called, flags; } tps_mod_row; /* 32 bytes */
typedef struct tps_mod_bin { uint16_t cpg, called, high, low; uint32_t sum; } tps_mod_bin;                                /* 12 bytes */
int  tps_batch_mod_profile(tps_ctx* ctx, int32_t slot, const uint8_t* tails, const int32_t* begin, const int32_t* end,
                           const int32_t* origin, int64_t n_reads, const int64_t* mod_off, const uint32_t* delta, const uint8_t* prob,
                           int64_t n_mods, int32_t w, int32_t nb0, int32_t nb1, int32_t hi, int32_t lo, tps_mod_row* rows,
                           int64_t rows_len, tps_mod_bin* bins, int64_t bins_len);

/* ---- measurement ----------------------------------------------------------------------- */
/* hipEvent timings of the scan kernel launches since the last reset: number of launches,
 * total and mean milliseconds (events are recorded on the stream the kernel runs on). */
int  tps_kernel_time_ms(tps_ctx* ctx, int32_t* n_launches, double* total_ms, double* mean_ms);
int  tps_kernel_time_reset(tps_ctx* ctx);
/* Diagnostics and tests only (ABI 4).  The library reads NO environment variables: what experiments and tests need to steer is
 * set per context through this call -- "event_stride" (time every n-th launch; default 1), "no_events", "force_generic" (the
 * generic kernel instead of the fused tiles), "spans_per_tile", "force_pair", "so_order", "wpg" (csrc/tps_plan.h: PlanKnobs), "lc_lds"
 * (0 = the default kernels write their change-point candidate sums off-chip like every other kernel; on by default: PlanKnobs::lc_lds), "stamps"
 * (per-read phase clocks; only a -DTPS_STAMPS build writes them), "file_order" (wave slot i takes read i: switches
 * tps::plan_dispatch_order off, which otherwise starts the longest reads of a batch first), "no_stride" (a slide that is a multiple of a
 * fused kernel's slide keeps the generic kernel instead of running that kernel and keeping every m-th window: tps::stride_base), "no_inline_rows" (such a scan at twice the base
 * slide copies its raw rows like the other multiples instead of letting the tiles store every second row: ScanArgs::raw_m), "poison"
 * (tests only; 0 = off, 1 .. 255 = a fill byte: while it is on, every call fills every device buffer it is about to use as output or
 * scratch with that byte, over the buffer's whole capacity and on the context's stream, ahead of its own clearing memsets and of the
 * launch, and the slot's mapped pinned result array likewise; buffers borrowed from another context or scan and inputs copied from the
 * host are never filled.  Two runs with different bytes differ exactly where nobody wrote what the call hands out).  topsicle_amd.hiplib applies $TOPSICLE_HIP_DEBUG
 * ("key=value,key=value") to every context it creates: the ONE documented variable of the Python host. */
int  tps_ctx_debug_option(tps_ctx* ctx, const char* key, int64_t value);
/* The stamps of the last scan of `slot`: 16 uint64 per read. */
int  tps_debug_stamps_get(tps_ctx* ctx, int32_t slot, uint64_t* out, int64_t n_reads);
/* Name of the device and a few properties, as a NUL-terminated string. */
int  tps_device_info(tps_ctx* ctx, char* buf, int32_t buf_len);
/* What the last tps_batch_scan of `slot` launched: "<kernel name> lds=<bytes per workgroup> wgs_per_cu=<n> waves_per_wg=<n>"
 * (the kernel family is chosen per scan from slide, table and LDS plan; profiles and bench.py name it).  A scan whose slide is a
 * multiple of a fused kernel's slide reports "<that kernel> every 2nd window" (3rd, 4th ...): it ran that kernel at the base slide
 * and kept every m-th window (tps_stride_kernel; outputs in the layout of the requested slide). */
int  tps_batch_kernel_info(tps_ctx* ctx, int32_t slot, char* buf, int32_t buf_len);

#ifdef __cplusplus
}
#endif
#endif /* TOPSICLE_HIP_H */
