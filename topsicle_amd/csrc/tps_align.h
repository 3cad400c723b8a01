// tps_align.h -- one window aligned base by base against another inside a band of 64 diagonals (tps_window_align): the distance, the
// path's two ends, the state of every reference column and, summed over the pairs of a pile row, the votes a consensus is called
// from.  Written against tps_wave.h like window_offsets_row (tps_anchor.h): one text for gfx950 and for the host emulation
// (tests/emu/emu_align.cpp), one 64-lane wave per pair.
//
// The rule (exact integers; include/topsicle_hip.h states it for the caller).  Q = the query's n letters, R = its reference row's m
// letters, c = centre.  Lane l owns the diagonal d = c - 32 + l: the cells (i, j) with j - i = d, 0 <= i <= n, 0 <= j <= m; every
// other cell is infinite.  D = 0 where i = 0 or j = 0; else D(i, j) = min(D(i-1, j-1) + [Q[i-1] != R[j-1]], D(i-1, j) + 1,
// D(i, j-1) + 1).  The end cell is the smallest D over the band cells with i = n or j = m, ties to the largest i, then the largest
// j.  The traceback prefers the diagonal, then up, then left, and stops at i = 0 or j = 0.
//
// How.  The wave walks the query's letters, one row of the band per step.
//   * up        D(i-1, j) lies on diagonal d + 1: lane l + 1 of the row before (one wave_shuffle).
//   * left      the chain inside a row is a prefix minimum over the lanes: with t = min(diagonal, up),
//               D[l] = min over l' <= l of t[l'] + (l - l') -- exact at unit cost.  t[l'] + 63 - l' goes through wave_incl_min_u32,
//               63 - l comes off again.  A cell beside the matrix is infinite before and after the chain.
//   * letters   both windows lie in the wave's LDS; a lane reads R[j-1] there, the row's Q[i-1] is wave-uniform, sixteen to a read.
//   * ends      a lane meets its one cell with j = m on the way and keeps its D; with the last row's that is two candidates per
//               lane, and the wave's smallest key D << 19 | (4096 - i) << 6 | (63 - l) is the end cell (on one row the larger j is
//               the larger lane).
//   * path      two ballots per row -- "the diagonal explains D", "else up does" -- are 16 bytes of the wave's LDS; the traceback
//               is wave-uniform code that reads them back and lane 0 writes the columns' states into a row of the same LDS.
//   * outputs   the columns leave in one coalesced store; the pile takes one integer atomic add per covered column and recorded
//               insertion (sums do not depend on order).
// The LDS is dynamic: the call sizes every wave's slice by its span and by the longest query that has a reference.
#pragma once
#include "../../include/topsicle_hip.h"
#include "tps_check.h"
#include "tps_wave.h"

namespace tps {

struct AlignArgs {
    const uint32_t* codes;       // [n][cdw] the queries
    const int32_t* length;       // [n]
    const uint32_t* ref_codes;   // [n_ref][cdw]
    const int32_t* ref_length;   // [n_ref]
    const int32_t* ref;          // [n] the reference row of query i, < 0: none
    const int32_t* centre;       // [n]
    const int32_t* pile_row;     // [n], or null
    int32_t* stat;               // [n][6]: every entry written
    uint16_t* cols;              // [n][span], or null: every entry written
    int32_t* pile;               // [n_pile][span][13], or null: cleared by the call, added to here
    int64_t n;
    int32_t span, cdw, rows;     // rows = align_rows(): what the path's ballots are sized for
};
constexpr int ALIGN_MAX_SPAN = 4096;
constexpr int64_t ALIGN_MAX_ROWS = 262144;
constexpr int ALIGN_BAND = 64, ALIGN_HALF = 32;            // lane l owns the diagonal centre - 32 + l
constexpr int ALIGN_STATS = 6, ALIGN_PILE = 13;            // dist, q_begin, q_end, r_begin, r_end, flags; A C T G del, ins1[4], ins2[4]
constexpr int ALIGN_NONE = 1, ALIGN_EDGE = 2;              // flags
constexpr uint32_t ALIGN_DELETED = 4, ALIGN_UNCOVERED = 7; // states of a column (0..3: the query's letter)
constexpr uint32_t ALIGN_INF = 1u << 20;
constexpr int ALIGN_WPG = 1;                               // waves per workgroup: no wave shares anything with its neighbour
static_assert(ALIGN_BAND == NT, "one lane per diagonal");
static_assert(ALIGN_MAX_SPAN < (1 << 13) && (uint64_t)ALIGN_MAX_SPAN << 19 < (1ull << 32), "the end cell's key fits 32 bits");

// one wave's LDS: the two windows' codes, the columns' states (16 bits each), four dwords of ballots per row
TPS_HD int align_cod_dw(int cdw) { return (cdw + 3) & ~3; }
TPS_HD int align_col_dw(int span) { return ((span + 1) / 2 + 3) & ~3; }
TPS_HD int align_lds_dw(int span, int cdw, int rows) { return 2 * align_cod_dw(cdw) + align_col_dw(span) + 4 * rows; }
static_assert(2 * (ALIGN_MAX_SPAN / 16) + ALIGN_MAX_SPAN / 2 + 4 * ALIGN_MAX_SPAN <= 160 * 1024 / 4, "the longest pair fits a CU's LDS");

// the rows of ballots the call's longest path needs: the longest query that has a reference, 1 at the least
static inline int align_rows(const int32_t* length, const int32_t* ref, int64_t n) {
    int rows = 1;
    for (int64_t i = 0; i < n; ++i)
        if (ref[i] >= 0 && length[i] > rows) rows = length[i];
    return rows;
}

// Every refusal of tps_window_align, in the library's order, the message in *why (host code; the library and the emulation call it).
// n = 0 needs no arrays.
static inline int window_align_check(const void* codes, int64_t codes_len, const int32_t* length, int64_t n, const void* ref_codes, int64_t ref_codes_len,
                                     const int32_t* ref_length, int64_t n_ref, const int32_t* ref, const int32_t* centre, int span, const void* stat,
                                     int64_t stat_len, const void* cols, int64_t cols_len, const int32_t* pile_row, const void* pile, int64_t n_pile,
                                     int64_t pile_len, Why* why) {
    if (n < 0 || n > ALIGN_MAX_ROWS) return refuse(why, TPS_E_CAPACITY, "n must be 0..262144");
    if (n_ref < 1 || n_ref > ALIGN_MAX_ROWS) return refuse(why, TPS_E_CAPACITY, "n_ref must be 1..262144");
    if (span < 1 || span > ALIGN_MAX_SPAN) return refuse(why, TPS_E_CAPACITY, "span must be 1..4096");
    if (n_pile < 0 || n_pile > n_ref) return refuse(why, TPS_E_CAPACITY, "n_pile must be 0..n_ref");
    const int64_t cdw = (span + 15) / 16;
    if (codes_len != n * cdw) return refuse(why, TPS_E_ARG, "codes must hold %lld dwords", (long long)(n * cdw));
    if (ref_codes_len != n_ref * cdw) return refuse(why, TPS_E_ARG, "ref_codes must hold %lld dwords", (long long)(n_ref * cdw));
    if (stat_len != n * ALIGN_STATS) return refuse(why, TPS_E_ARG, "stat must hold %lld entries", (long long)(n * ALIGN_STATS));
    if (cols_len != (cols ? n * span : 0)) return refuse(why, TPS_E_ARG, "cols must hold %lld entries", (long long)(cols ? n * span : 0));
    if (pile && n_pile == 0) return refuse(why, TPS_E_ARG, "a pile needs n_pile of 1 or more");
    if (n_pile > 0 && !pile_row) return refuse(why, TPS_E_ARG, "n_pile rows need pile_row");
    if (pile_len != (pile ? n_pile * span * ALIGN_PILE : 0)) return refuse(why, TPS_E_ARG, "pile must hold %lld entries", (long long)(pile ? n_pile * span * ALIGN_PILE : 0));
    if (n == 0) return TPS_OK;
    if (!codes || !length || !ref_codes || !ref_length || !ref || !centre || !stat) return refuse(why, TPS_E_ARG, "null codes / length / ref_codes / ref_length / ref / centre / stat");
    for (int64_t r = 0; r < n_ref; ++r)
        if (ref_length[r] < 0 || ref_length[r] > span) return refuse(why, TPS_E_ARG, "reference row %lld: length must be 0..span", (long long)r);
    for (int64_t i = 0; i < n; ++i) {
        if (length[i] < 0 || length[i] > span) return refuse(why, TPS_E_ARG, "row %lld: length must be 0..span", (long long)i);
        if (ref[i] >= n_ref) return refuse(why, TPS_E_ARG, "row %lld: ref must be below n_ref (negative: no reference)", (long long)i);
        if (centre[i] < -ALIGN_MAX_SPAN || centre[i] > ALIGN_MAX_SPAN) return refuse(why, TPS_E_ARG, "row %lld: centre must be -4096..4096", (long long)i);
        if (pile_row && pile_row[i] >= n_pile) return refuse(why, TPS_E_ARG, "row %lld: pile_row must be below n_pile (negative: not counted)", (long long)i);
    }
    return TPS_OK;
}

// letter p of a staged window (p inside it)
TPS_DEV uint32_t align_letter(const uint32_t* cod, int p) { return (cod[p >> 4] >> (2 * (p & 15))) & 3u; }

// row i without an alignment: NONE, all numbers 0, every column "not covered" (wave code)
TPS_DEV void align_none(const AlignArgs& a, int64_t i) {
    TPS_PHASE {
        if (tid < ALIGN_STATS) a.stat[i * ALIGN_STATS + tid] = tid == ALIGN_STATS - 1 ? ALIGN_NONE : 0;
        if (a.cols)
            for (int c = tid; c < a.span; c += NT) a.cols[i * a.span + c] = (uint16_t)ALIGN_UNCOVERED;
    }
}

// pair i; `lds`: align_lds_dw(span, cdw, rows) dwords of the wave's own
TPS_DEV void window_align_row(const AlignArgs& a, int64_t i, uint32_t* lds) {
    const int64_t ref = a.ref[i];
    if (ref < 0) { align_none(a, i); return; }
    const int cod_dw = align_cod_dw(a.cdw);
    uint32_t* rcod = lds;
    uint32_t* qcod = lds + cod_dw;
    uint16_t* col = (uint16_t*)(lds + 2 * cod_dw);
    uint32_t* dir = lds + 2 * cod_dw + align_col_dw(a.span);
    const int n = a.length[i], m = a.ref_length[ref];
    const int d0 = a.centre[i] - ALIGN_HALF;               // lane 0's diagonal
    TPS_PHASE {
        for (int c = tid; c < a.cdw; c += NT) {
            rcod[c] = a.ref_codes[ref * a.cdw + c];
            qcod[c] = a.codes[i * a.cdw + c];
        }
        for (int c = tid; c < a.span; c += NT) col[c] = (uint16_t)ALIGN_UNCOVERED;
    }
    TPS_SYNC();
    // row 0, and a lane's cell with j = m where that is on row 0
    Lane<uint32_t> P, E;
    TPS_PHASE {
        const int j = d0 + tid;
        TPS_AT(P) = j >= 0 && j <= m ? 0u : ALIGN_INF;
        TPS_AT(E) = j == m ? 0u : ALIGN_INF;
    }
    const int ln = tps_fresh_lane();
    uint32_t qw = 0;                                       // sixteen of the query's letters: one wave-uniform LDS read per 16 rows
    for (int r = 1; r <= n; ++r) {
        if (((r - 1) & 15) == 0) qw = uniform(qcod[(r - 1) >> 4]);
        const uint32_t q = (qw >> (2 * ((r - 1) & 15))) & 3u;
        Lane<uint32_t> T, DG, UP;
        TPS_PHASE_WITH(ln) {
            const int j = r + d0 + tid;
            const bool in = j >= 1 && j <= m;
            const uint32_t above = wave_shuffle(P, tid, tid < NT - 1 ? tid + 1 : tid);
            const uint32_t rl = align_letter(rcod, in ? j - 1 : 0);
            const uint32_t dg = TPS_AT(P) + (rl != q ? 1u : 0u);
            const uint32_t up = (tid < NT - 1 ? above : ALIGN_INF) + 1u;
            uint32_t t = dg < up ? dg : up;
            t = t < ALIGN_INF ? t : ALIGN_INF;
            t = in ? t : j == 0 ? 0u : ALIGN_INF;
            TPS_AT(DG) = dg;
            TPS_AT(UP) = up;
            TPS_AT(T) = t + (uint32_t)(NT - 1 - tid);
        }
        const Lane<uint32_t> M = wave_incl_min_u32(T);
        Lane<bool> by_dg, by_up;
        TPS_PHASE_WITH(ln) {
            const int j = r + d0 + tid;
            uint32_t d = TPS_AT(M) - (uint32_t)(NT - 1 - tid);
            d = d < ALIGN_INF && j >= 0 && j <= m ? d : ALIGN_INF;
            TPS_AT(by_dg) = d < ALIGN_INF && d == TPS_AT(DG);
            TPS_AT(by_up) = d < ALIGN_INF && d != TPS_AT(DG) && d == TPS_AT(UP);
            TPS_AT(P) = d;
            if (j == m) TPS_AT(E) = d;
        }
        const uint64_t bd = wave_ballot(by_dg), bu = wave_ballot(by_up);
        TPS_PHASE_WITH(ln) {
            if (tid < 4) dir[4 * (r - 1) + tid] = (uint32_t)((tid < 2 ? bd : bu) >> (32 * (tid & 1)));
        }
    }
    // the end cell: the smallest D << 19 | (4096 - i) << 6 | (63 - lane) of the last row's cells and of the cells with j = m
    Lane<uint32_t> key;
    TPS_PHASE {
        const int ie = m - d0 - tid;                       // the row of this lane's cell with j = m
        const uint32_t k1 = TPS_AT(P) < ALIGN_INF ? (TPS_AT(P) << 19) | ((uint32_t)(ALIGN_MAX_SPAN - n) << 6) | (uint32_t)(NT - 1 - tid) : 0xFFFFFFFFu;
        const uint32_t k2 = ie >= 0 && ie <= n && TPS_AT(E) < ALIGN_INF ? (TPS_AT(E) << 19) | ((uint32_t)(ALIGN_MAX_SPAN - ie) << 6) | (uint32_t)(NT - 1 - tid) : 0xFFFFFFFFu;
        TPS_AT(key) = ~(k1 < k2 ? k1 : k2);
    }
    const uint32_t best = ~wave_max_u32(key);
    if (best == 0xFFFFFFFFu) { align_none(a, i); return; }       // the band misses the matrix
    TPS_SYNC();
    const int dist = (int)(best >> 19), q_end = ALIGN_MAX_SPAN - (int)((best >> 6) & 8191u);
    int l = NT - 1 - (int)(best & 63u);
    const int r_end = q_end + d0 + l;
    int ci = q_end, cj = r_end, flags = 0;
    uint32_t ins_n = 0, ins_1 = 0, ins_2 = 0;              // the inserted letters in front of column cj, as met so far
    while (ci > 0 && cj > 0) {
        if (l == 0 || l == NT - 1) flags |= ALIGN_EDGE;
        const uint32_t bit = 1u << (l & 31);
        const bool by_dg = (uniform(dir[4 * (ci - 1) + (l >> 5)]) & bit) != 0;
        const bool by_up = (uniform(dir[4 * (ci - 1) + 2 + (l >> 5)]) & bit) != 0;
        if (by_up) {                               // Q[ci - 1] stands in front of column cj: the letters come last one first
            ins_2 = ins_1;
            ins_1 = uniform(align_letter(qcod, ci - 1));
            ++ins_n;
            --ci;
            ++l;
            continue;
        }
        // column cj - 1 takes a letter or is deleted; the insertions in front of cj lie between two covered columns unless cj is the end
        const uint32_t state = by_dg ? uniform(align_letter(qcod, ci - 1)) : ALIGN_DELETED;
        const uint32_t ins = ins_n && cj < r_end ? ((ins_n < 3 ? ins_n : 3u) << 3) | (ins_1 << 5) | ((ins_n >= 2 ? ins_2 : 0u) << 7) : 0u;
        const bool put_ins = ins != 0;
        TPS_PHASE {
            if (tid == 0) {
                col[cj - 1] = (uint16_t)state;
                if (put_ins) col[cj] = (uint16_t)(col[cj] | ins);
            }
        }
        ins_n = 0;
        --cj;
        if (by_dg) --ci;
        else --l;
    }
    TPS_SYNC();
    const int q_begin = ci, r_begin = cj;
    const int64_t prow = a.pile && a.pile_row && flags == 0 ? (int64_t)a.pile_row[i] : -1;
    TPS_PHASE {
        if (tid < ALIGN_STATS)
            a.stat[i * ALIGN_STATS + tid] = tid == 0 ? dist : tid == 1 ? q_begin : tid == 2 ? q_end : tid == 3 ? r_begin : tid == 4 ? r_end : flags;
        if (a.cols)
            for (int c = tid; c < a.span; c += NT) a.cols[i * a.span + c] = col[c];
        if (prow >= 0) {
            int32_t* pile = a.pile + prow * a.span * ALIGN_PILE;
            for (int c = r_begin + tid; c < r_end; c += NT) {
                const uint32_t v = col[c];
                g_add_i32(&pile[c * ALIGN_PILE + (int)(v & 7u)], 1);
                if ((v >> 3) & 3u) g_add_i32(&pile[c * ALIGN_PILE + 5 + (int)((v >> 5) & 3u)], 1);
                if (((v >> 3) & 3u) >= 2) g_add_i32(&pile[c * ALIGN_PILE + 9 + (int)((v >> 7) & 3u)], 1);
            }
        }
    }
}

}  // namespace tps
