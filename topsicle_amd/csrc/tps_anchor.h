// tps_anchor.h -- anchored telomere lengths: the kept window of every read as packed letters and keep bits (tps_batch_end_window),
// and the offset of one window against another by votes on their diagonals (tps_window_offsets).  Written against tps_wave.h like
// end_sketch_read (tps_ends.h): one text for gfx950 and for the host emulation (tests/emu/emu_anchor.cpp), one 64-lane wave per
// read / per query row.
//
// The kept window (exact; include/topsicle_hip.h states it for the caller).  The sketch's string h, its window [begin, min(end, L)),
// its k and its KEPT rule.  codes[r]: the window's letters as 2-bit codes, 16 per dword, complemented for tail 1, a letter that is
// not ACGT and everything behind the window 0.  keep[r]: bit q set exactly when the k-mer at begin + q is KEPT.
//
// How.  The window is walked in the sketch's pieces (ENDS_PIECE k-mer positions, k - 1 bases of overlap) with the sketch's staging
// and word ballots; a step's keep flags are one ballot = two dwords of the keep row, and 16 letters of the staged string are one
// dword of the codes row, masked where the invalid words say so and behind the window's last letter.  Both rows are put together in
// the wave's LDS (the sketch's bucket area) and leave in one coalesced store each, zeros behind the window included.  The keep
// predicate is the sketch's own function (ends_keep, tps_ends.h); taking it out of end_sketch_read left that kernel's instructions
// as they were (the same assembly, line for line).
//
// The offset rule.  x = fmix32(c ^ 0x9E3779B9) of a kept k-mer.  Table of the reference window R: 4096 slots, slot x >> 20 holds the
// smallest ((x & 0xFFFFF) << 12) | q over R's kept positions q.  A kept position p of the query Q whose slot holds its own low 20
// bits votes for the diagonal d = q - p.  Coarse: 128 bins of 64 diagonals, pair[c] = H[c] + H[c + 1], best = the smallest c with
// the largest pair, second = the largest pair at least two bins away.  Fine: the 128 diagonals of the best pair, offset = their
// lower median.
//
// How.  One wave per query row; its LDS holds the table (16 KB), the two histograms and ONE window's codes and keep words: the
// reference is staged, hashed into the table with one LDS atomic minimum per kept k-mer, then the query takes its place.  64
// positions are one step; a step whose 64 keep bits are clear is skipped, a lane whose bit is clear sits it out.  The query is
// walked twice (coarse votes, then the fine histogram of the best pair): the table look-ups are repeated instead of 4096 diagonals
// being kept.  The maxima are wave reductions of (pair << 7 | 127 - c), the median is a prefix sum over the lanes' bin pairs.
#pragma once
#include "tps_ends.h"

namespace tps {

struct EndWindowArgs {
    const uint32_t* seq2;
    const uint16_t* inv;
    const tps_read_desc* desc;
    const uint32_t* table;       // tract_hit_table(unit, m); the device kernel reads its copy in LDS
    const uint8_t* tails;        // [n_reads] 0 / 1
    const int32_t* begin;        // [n_reads]
    const int32_t* end;          // [n_reads]
    uint32_t* codes;             // [n_reads][cdw]: every entry written
    uint32_t* keep;              // [n_reads][kdw]: every entry written
    int64_t n_reads;
    int32_t w, k, cdw, kdw;      // cdw = (span + 15) / 16, kdw = (span + 31) / 32
};
struct OffsetArgs {
    const uint32_t* codes;       // [n][cdw]
    const uint32_t* keep;        // [n][kdw]
    const int32_t* length;       // [n] letters of the window
    const int32_t* ref;          // [n] the row whose window is the reference, < 0: none
    int32_t* offset;             // [n]: every entry written, like the two below
    int32_t* votes;
    int32_t* second;
    int64_t n;
    int32_t k, cdw, kdw;
};
constexpr int ANCHOR_MAX_SPAN = 4096;
constexpr int64_t ANCHOR_MAX_ROWS = 262144;
constexpr int ANCHOR_SLOTS = 4096;                         // of the reference's table: the top 12 bits of a hash
constexpr int ANCHOR_BINS = 128;                           // coarse: 64 diagonals each; fine: one each
constexpr int ANCHOR_ROW_CDW = ANCHOR_MAX_SPAN / 16, ANCHOR_ROW_KDW = ANCHOR_MAX_SPAN / 32;
constexpr int WINDOW_OUT_OFF = ENDS_BKT_OFF;               // the window kernel builds its two rows where the sketch keeps its buckets
constexpr int OFFSETS_COD_DW = ANCHOR_ROW_CDW + 4;         // (v_at reads a dword ahead)
constexpr int OFFSETS_H_OFF = ANCHOR_SLOTS, OFFSETS_F_OFF = OFFSETS_H_OFF + ANCHOR_BINS, OFFSETS_COD_OFF = OFFSETS_F_OFF + ANCHOR_BINS;
constexpr int OFFSETS_KEEP_OFF = OFFSETS_COD_OFF + OFFSETS_COD_DW;
constexpr int OFFSETS_LDS_DW = OFFSETS_KEEP_OFF + ANCHOR_ROW_KDW;       // per wave: 4740 dwords
// Waves per workgroup.  No wave shares anything with its neighbour, so the size of a group only decides how the CU's 160 KiB are cut:
// a wave's 18 960 bytes allow eight waves per CU either way, and two of them stay under the 64 KiB of a static array (four: 75 840).
constexpr int OFFSETS_WPG = 2;
static_assert(ANCHOR_ROW_CDW + ANCHOR_ROW_KDW <= ENDS_MAX_BUCKETS, "the two rows fit the sketch's bucket area");
static_assert(ENDS_PIECE % 32 == 0 && ANCHOR_MAX_SPAN <= 2 * ENDS_PIECE, "a piece ends on a dword of both rows; two pieces at most");
static_assert(OFFSETS_LDS_DW % 4 == 0 && OFFSETS_COD_OFF % 4 == 0, "every wave's table starts on a 16-byte boundary (lds_store16)");
static_assert(ANCHOR_MAX_SPAN - ENDS_MIN_K < (1 << 12) && 2 * ANCHOR_MAX_SPAN == 64 * ANCHOR_BINS, "a position fits 12 bits, the diagonals the bins");

// The checks of tps_batch_end_window behind those of the sketch (ends_check, ends_check_reads), and those of tps_window_offsets
// (host code; the library and the emulation share them): TPS_OK, or the code and *why.
static inline int window_check_span(int span, int k, const char** why) {
    if (span < k || span > ANCHOR_MAX_SPAN) { *why = "span must be k..4096"; return TPS_E_CAPACITY; }
    return TPS_OK;
}
static inline int window_check_reads(const int32_t* begin, const int32_t* end, int64_t n, int span, const char** why, int64_t* at) {
    for (int64_t i = 0; i < n; ++i) {
        *at = i;
        if ((int64_t)end[i] - begin[i] > span) { *why = "end - begin must be at most span"; return TPS_E_CAPACITY; }
    }
    return TPS_OK;
}
static inline int offsets_check(int64_t n, int span, int k, int64_t out_len, const char** why) {
    if (k < ENDS_MIN_K || k > ENDS_MAX_K) { *why = "k must be 8..16"; return TPS_E_CAPACITY; }
    if (span < k || span > ANCHOR_MAX_SPAN) { *why = "span must be k..4096"; return TPS_E_CAPACITY; }
    if (n < 0 || n > ANCHOR_MAX_ROWS) { *why = "n must be 0..262144"; return TPS_E_CAPACITY; }
    if (out_len != n) { *why = "offset, votes and second must hold n entries"; return TPS_E_ARG; }
    return TPS_OK;
}
static inline int offsets_check_rows(const int32_t* length, const int32_t* ref, int64_t n, int span, const char** why, int64_t* at) {
    for (int64_t i = 0; i < n; ++i) {
        *at = i;
        if (ref[i] >= n) { *why = "ref must be below n (negative: no reference)"; return TPS_E_ARG; }
        if (length[i] < 0 || length[i] > span) { *why = "length must be 0..span"; return TPS_E_ARG; }
    }
    return TPS_OK;
}

// Every refusal of tps_batch_end_window and of tps_window_offsets that needs no context, in the library's order, the message in *why
// (host code; the library and the emulation call them).  n = the reads of the batch, the rows of the call; n = 0 needs no arrays.
static inline int end_window_check(int64_t n, uint64_t unit, int m, int k, const uint8_t* tails, const int32_t* begin, const int32_t* end, int64_t n_reads,
                                   int span, const void* codes, int64_t codes_len, const void* keep, int64_t keep_len, Why* why) {
    const char* s = "";
    int64_t at = 0;
    if (const int rc = ends_check(unit, m, k, ENDS_MIN_BUCKETS, &s)) return refuse(why, rc, "%s", s);
    if (const int rc = window_check_span(span, k, &s)) return refuse(why, rc, "%s", s);
    const int cdw = (span + 15) / 16, kdw = (span + 31) / 32;
    if (n_reads != n) return refuse(why, TPS_E_ARG, "tails, begin and end must hold %lld reads", (long long)n);
    if (codes_len != n * cdw) return refuse(why, TPS_E_ARG, "codes must hold %lld dwords", (long long)(n * cdw));
    if (keep_len != n * kdw) return refuse(why, TPS_E_ARG, "keep must hold %lld dwords", (long long)(n * kdw));
    if (n == 0) return TPS_OK;
    if (!tails || !begin || !end || !codes || !keep) return refuse(why, TPS_E_ARG, "null tails / begin / end / codes / keep");
    if (const int rc = ends_check_reads(tails, begin, end, n, &s, &at)) return refuse(why, rc, "read %lld: %s", (long long)at, s);
    if (const int rc = window_check_reads(begin, end, n, span, &s, &at)) return refuse(why, rc, "read %lld: %s", (long long)at, s);
    return TPS_OK;
}
static inline int window_offsets_check(const void* codes, const void* keep, const int32_t* length, const int32_t* ref, int64_t n, int span, int k,
                                       const void* offset, const void* votes, const void* second, int64_t out_len, Why* why) {
    const char* s = "";
    int64_t at = 0;
    if (const int rc = offsets_check(n, span, k, out_len, &s)) return refuse(why, rc, "%s", s);
    if (n == 0) return TPS_OK;
    if (!codes || !keep || !length || !ref || !offset || !votes || !second) return refuse(why, TPS_E_ARG, "null codes / keep / length / ref / offset / votes / second");
    if (const int rc = offsets_check_rows(length, ref, n, span, &s, &at)) return refuse(why, rc, "row %lld: %s", (long long)at, s);
    return TPS_OK;
}

// the 16 bits of x, bit j at bits 2j and 2j + 1
TPS_DEV uint32_t anchor_pairs(uint32_t x) {
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x * 3u;
}

// `tab`: the hit table (device: the workgroup's copy in LDS); `lds`: one wave's slice of the sketch's layout
TPS_DEV void end_window_read(const EndWindowArgs& a, int64_t r, uint32_t* lds, const uint32_t* tab) {
    uint32_t* seq = lds;
    uint16_t* val = (uint16_t*)(lds + FOLLOW_SEQ_DW);
    uint32_t* oc = lds + WINDOW_OUT_OFF;                   // the codes row
    uint32_t* ok = oc + ANCHOR_ROW_CDW;                    // the keep row
    uint32_t* misc = lds + ENDS_MISC_OFF;
    const int64_t woff = a.desc[r].word_off;
    const int64_t L = a.desc[r].len;
    const bool has_inv = (a.desc[r].flags & TPS_RD_HAS_INVALID) != 0;
    const int k = a.k, w = a.w;
    const int64_t b = a.begin[r];
    const int64_t e = (int64_t)a.end[r] < L ? (int64_t)a.end[r] : L;
    const bool rev = a.tails[r] != 0;
    const uint32_t flip = rev ? 0xAAAAAAAAu : 0u;          // complement: A <-> T, C <-> G is code ^ 2
    const uint32_t cmask = (1u << (2 * w)) - 1u;
    const uint64_t bad_bits = (1ull << k) - 1ull;
    const uint64_t wbits = (1ull << (k - w + 1)) - 1ull;   // the words of one k-mer
    const int64_t nlet = e - b;                            // letters of the window (<= 0: none; <= span: the host checks)
    const int64_t npos = nlet - k + 1;                     // k-mer positions of the window (<= 0: none)
    TPS_PHASE {
        for (int c = tid; c < ANCHOR_ROW_CDW + ANCHOR_ROW_KDW; c += NT) oc[c] = 0;
    }
    TPS_SYNC();
    for (int64_t lo = 0; lo < nlet; lo += ENDS_PIECE) {
        const int nc = (int)(nlet - lo < ENDS_PIECE ? nlet - lo : ENDS_PIECE);             // letters whose codes this piece writes
        const int nl = (int)(nlet - lo < ENDS_PIECE + k - 1 ? nlet - lo : ENDS_PIECE + k - 1);     // letters it stages
        const int np = (int)(npos - lo < 0 ? 0 : npos - lo < ENDS_PIECE ? npos - lo : ENDS_PIECE);   // k-mer positions it decides
        const int nwords = np + k - w;
        const Stage st = stage_plan(a.seq2, a.inv, woff, L, rev, 0, b + lo, nl);
        TPS_PHASE { if (tid == 0) misc[M_INVALID] = 0; }
        TPS_SYNC();
        // (+ two quads of zeros: the lanes of the step behind the last one read there, v_at a word ahead)
        TPS_PHASE { stage_thread(st, has_inv, seq, val, st.nq + 2, &misc[M_INVALID], tid); }
        TPS_SYNC();
        const bool any_inv = has_inv && uniform(misc[M_INVALID]) != 0;
        const int cbase = (int)(lo >> 4);
        TPS_PHASE {
            for (int j = tid; 16 * j < nc; j += NT) {
                const int q = st.delta + 16 * j;
                uint32_t bad = 0;
                if (any_inv) {
                    const int idx = q >> 4;
                    bad = ((((uint32_t)val[idx] | ((uint32_t)val[idx + 1] << 16)) >> (q & 15)) & 0xFFFFu);
                }
                const int left = nc - 16 * j;              // letters of this dword inside the window
                if (left < 16) bad |= (0xFFFFu << left) & 0xFFFFu;
                oc[cbase + j] = (v_at(seq, q) ^ flip) & ~anchor_pairs(bad);
            }
        }
        if (np > 0) {
            const int steps = (np + NT - 1) / NT;
            const int kbase = (int)(lo >> 5);
            const int ln = tps_fresh_lane();
            uint64_t nxt = ends_word_ballot(seq, tab, st.delta, 0, nwords, flip, cmask, ln);
            for (int s = 0; s < steps; ++s) {
                const uint64_t cur = nxt;
                nxt = ends_word_ballot(seq, tab, st.delta, s + 1, nwords, flip, cmask, ln);
                Lane<bool> kp;
                TPS_PHASE_WITH(ln) {
                    const int t = s * NT + tid;
                    TPS_AT(kp) = ends_keep(cur, nxt, wbits, t, np, any_inv, val, st.delta + t, bad_bits, tid);
                }
                const uint64_t bal = wave_ballot(kp);
                TPS_PHASE_WITH(ln) {
                    if (tid < 2) ok[kbase + 2 * s + tid] = (uint32_t)(bal >> (32 * tid));
                }
            }
        }
        TPS_SYNC();                                // the next piece overwrites what this one's lanes read
    }
    TPS_SYNC();
    TPS_PHASE {
        for (int c = tid; c < a.cdw; c += NT) a.codes[r * a.cdw + c] = oc[c];
        for (int c = tid; c < a.kdw; c += NT) a.keep[r * a.kdw + c] = ok[c];
    }
}

// one window's rows into the wave's LDS, zeros behind them
TPS_DEV void offsets_stage(const OffsetArgs& a, int64_t row, uint32_t* cod, uint32_t* kp) {
    TPS_PHASE {
        for (int c = tid; c < OFFSETS_COD_DW; c += NT) cod[c] = c < a.cdw ? a.codes[row * a.cdw + c] : 0u;
        for (int c = tid; c < ANCHOR_ROW_KDW; c += NT) kp[c] = c < a.kdw ? a.keep[row * a.kdw + c] : 0u;
    }
}
// the hash of the kept k-mer at position p of the staged window; false: none (the lane sits the step out)
TPS_DEV bool offsets_kmer(const uint32_t* cod, const uint32_t* kp, int p, int npos, uint32_t kmask, uint32_t& x) {
    if (p >= npos || ((kp[p >> 5] >> (p & 31)) & 1u) == 0) return false;
    x = ends_fmix32((v_at(cod, p) & kmask) ^ 0x9E3779B9u);
    return true;
}
// ... and the diagonal it votes for; false: no vote
TPS_DEV bool offsets_vote(const uint32_t* tbl, const uint32_t* cod, const uint32_t* kp, int p, int npos, uint32_t kmask, int& d) {
    uint32_t x;
    if (!offsets_kmer(cod, kp, p, npos, kmask, x)) return false;
    const uint32_t t = tbl[x >> 20];
    if (t == ENDS_EMPTY || (t >> 12) != (x & 0xFFFFFu)) return false;
    d = (int)(t & 4095u) - p;
    return true;
}
// are the 64 keep bits of step s clear?  (wave-uniform)
TPS_DEV bool offsets_step_empty(const uint32_t* kp, int s) { return (uniform(kp[2 * s]) | uniform(kp[2 * s + 1])) == 0; }

// coarse: best = the smallest c with the largest pair, votes = that pair, second = the largest pair at least two bins away (wave code)
TPS_DEV void offsets_best(const uint32_t* H, int& best, uint32_t& votes, uint32_t& second) {
    // the smallest c with the largest pair: the maximum of pair << 7 | 127 - c (a pair is at most 4096 votes)
    Lane<uint32_t> key, sec;
    TPS_PHASE {
        uint32_t m = 0;
        for (int c = tid; c < ANCHOR_BINS - 1; c += NT) {
            const uint32_t kc = ((H[c] + H[c + 1]) << 7) | (uint32_t)(ANCHOR_BINS - 1 - c);
            m = kc > m ? kc : m;
        }
        TPS_AT(key) = m;
    }
    const uint32_t top = wave_max_u32(key);
    best = ANCHOR_BINS - 1 - (int)(top & 127u);
    votes = top >> 7;
    const int b = best;
    TPS_PHASE {
        uint32_t m = 0;
        for (int c = tid; c < ANCHOR_BINS - 1; c += NT) {
            const uint32_t pr = H[c] + H[c + 1];
            if ((c >= b + 2 || c <= b - 2) && pr > m) m = pr;
        }
        TPS_AT(sec) = m;
    }
    second = wave_max_u32(sec);
}
// fine: *out = the lower median of the votes (> 0) counted in F, the 128 diagonals from dlo on (wave code; one lane stores)
TPS_DEV void offsets_median(const uint32_t* F, uint32_t votes, int dlo, int32_t* out) {
    // the diagonal that holds vote (votes - 1) / 2 of the sorted ones; a lane looks at two neighbouring diagonals
    Lane<uint32_t> two;
    TPS_PHASE { TPS_AT(two) = F[2 * tid] + F[2 * tid + 1]; }
    const Lane<uint32_t> before = wave_excl_sum(two);
    const uint32_t mid = (votes - 1u) / 2u;
    TPS_PHASE {
        const uint32_t e0 = TPS_AT(before), f0 = F[2 * tid];
        if (mid >= e0 && mid < e0 + TPS_AT(two)) *out = dlo + 2 * tid + (mid >= e0 + f0 ? 1 : 0);
    }
}

// row i of the offsets; `lds`: OFFSETS_LDS_DW dwords of the wave's own
TPS_DEV void window_offsets_row(const OffsetArgs& a, int64_t i, uint32_t* lds) {
    uint32_t* tbl = lds;
    uint32_t* H = lds + OFFSETS_H_OFF;
    uint32_t* F = lds + OFFSETS_F_OFF;
    uint32_t* cod = lds + OFFSETS_COD_OFF;
    uint32_t* kp = lds + OFFSETS_KEEP_OFF;
    const int64_t ref = a.ref[i];
    if (ref < 0) {
        TPS_PHASE { if (tid == 0) { a.offset[i] = 0; a.votes[i] = 0; a.second[i] = 0; } }
        return;
    }
    const int k = a.k;
    const uint32_t kmask = 0xFFFFFFFFu >> (32 - 2 * k);
    const int npos_r = a.length[ref] - k + 1, npos_q = a.length[i] - k + 1;
    const int steps_r = npos_r > 0 ? (npos_r + NT - 1) / NT : 0, steps_q = npos_q > 0 ? (npos_q + NT - 1) / NT : 0;
    TPS_PHASE {
        u32x4 em;
        em.x = em.y = em.z = em.w = ENDS_EMPTY;
        for (int c = tid; c < ANCHOR_SLOTS / 4; c += NT) lds_store16(tbl + 4 * c, em);
        for (int c = tid; c < 2 * ANCHOR_BINS; c += NT) H[c] = 0;          // (F lies behind H)
    }
    offsets_stage(a, ref, cod, kp);
    TPS_SYNC();
    const int ln = tps_fresh_lane();
    for (int s = 0; s < steps_r; ++s) {
        if (offsets_step_empty(kp, s)) continue;
        TPS_PHASE_WITH(ln) {
            const int q = s * NT + tid;
            uint32_t x;
            if (offsets_kmer(cod, kp, q, npos_r, kmask, x)) lds_min_u32(&tbl[x >> 20], ((x & 0xFFFFFu) << 12) | (uint32_t)q);
        }
    }
    TPS_SYNC();
    if (ref != i) {                                // (its own reference: the window is in place)
        offsets_stage(a, i, cod, kp);
        TPS_SYNC();
    }
    for (int s = 0; s < steps_q; ++s) {
        if (offsets_step_empty(kp, s)) continue;
        TPS_PHASE_WITH(ln) {
            int d;
            if (offsets_vote(tbl, cod, kp, s * NT + tid, npos_q, kmask, d)) lds_add(&H[(d + ANCHOR_MAX_SPAN) >> 6], 1u);
        }
    }
    TPS_SYNC();
    int best;
    uint32_t votes, second;
    offsets_best(H, best, votes, second);
    if (votes != 0) {
        const int dlo = 64 * best - ANCHOR_MAX_SPAN;
        for (int s = 0; s < steps_q; ++s) {
            if (offsets_step_empty(kp, s)) continue;
            TPS_PHASE_WITH(ln) {
                int d;
                if (offsets_vote(tbl, cod, kp, s * NT + tid, npos_q, kmask, d) && (uint32_t)(d - dlo) < (uint32_t)ANCHOR_BINS) lds_add(&F[d - dlo], 1u);
            }
        }
        TPS_SYNC();
        offsets_median(F, votes, dlo, &a.offset[i]);
    }
    TPS_PHASE {
        if (tid == 0) {
            if (votes == 0) a.offset[i] = 0;
            a.votes[i] = (int32_t)votes;
            a.second[i] = (int32_t)second;
        }
    }
}

}  // namespace tps
