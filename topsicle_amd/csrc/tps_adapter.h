// tps_adapter.h -- adapters at the telomere end of a read (tps_batch_adapter_find): the smallest unit-cost edit distance between
// each of up to 64 given sequences and any substring of a region of the read, and where the best occurrence ends.  The first
// approximate matcher of the library.  Written against tps_wave.h like variant_read (tps_variant.h) and end_window_read
// (tps_anchor.h): one text for gfx950 and for the host emulation (tests/emu/emu_adapter.cpp), one 64-lane wave per read, no pattern
// table.
//
// The rule (exact integers; include/topsicle_hip.h states it for the caller).  h = the upper-cased read (tail 0) or its reverse
// complement (tail 1); the region T = h[begin .. min(end, L)), n = |T| <= 1024.  For pattern A_j of m_j letters, D_j(e), e = 0 .. n,
// is the smallest edit distance (substitution, insertion, deletion: 1 each) between A_j and any T[s .. e), s <= e -- Sellers'
// recurrence, D[0][e] = 0, D[i][0] = i; a letter of T that is not ACGT matches nothing.  dist_j = min over e of D_j(e), end_j = the
// smallest e that reaches it; an empty region gives (m_j, 0).
//
// How.  Lane j owns pattern j and runs Myers' bit-vector recurrence in the approximate-search form over the n letters: the column
// of vertical deltas as the two 64-bit words Pv / Mv, bit i = row i + 1, the four match masks Peq[c] of its pattern (bit i set where
// A_j[i] has code c; the host builds them once per call, adapter_build_peq), the score of the last row, and the best (score, e) so
// far, replaced on a strict improvement only -- which is what makes end_j the smallest e.  The horizontal delta shifted in at bit 0
// is 0 (row 0 of the search form is all zeros), and the score follows bit m_j - 1 of the horizontal deltas.  The region is staged
// once with stage_plan / stage_thread as end_window_read does it: tail 1 is staged reversed and the codes are complemented here
// (code ^ 2), the invalid words mark the letters that are not ACGT, for which Eq = 0.  The letter of a step is the same for every
// lane: the staged dword (16 letters) and its invalid word are read once per 16 steps through uniform() and the Peq word is selected
// by the scalar code.  The loop runs n times, n bounded by the host (ADAPTER_MAX_REGION): no loop's length depends on the data.  Lanes
// at or past n_pat sit out and store nothing; lane j stores dist | end << 16, the (dist, end) pair of uint16 the caller reads.
#pragma once
#include "tps_device.h"

namespace tps {

struct AdapterArgs {
    const uint32_t* seq2;
    const uint16_t* inv;
    const tps_read_desc* desc;
    const uint64_t* peq;         // [n_pat][4]: adapter_build_peq
    const int32_t* pat_len;      // [n_pat]
    const uint8_t* tails;        // [n_reads] 0 / 1
    const int32_t* begin;        // [n_reads]
    const int32_t* end;          // [n_reads]
    uint32_t* hits;              // [n_reads][n_pat]: dist | end << 16, every entry written
    int64_t n_reads;
    int32_t n_pat;
};
constexpr int ADAPTER_MIN_LEN = 12, ADAPTER_MAX_LEN = 64;  // letters of a pattern: one bit each of a 64-bit word
constexpr int ADAPTER_MAX_PATTERNS = NT;                   // one lane each
constexpr int ADAPTER_MAX_REGION = 1024;
// the staging area: the region from any place in its first quad on (delta <= 63), in whole quads; the invalid words, 8 bytes per quad
constexpr int ADAPTER_QUADS = (63 + ADAPTER_MAX_REGION + 63) / 64;
constexpr int ADAPTER_SEQ_DW = 4 * ADAPTER_QUADS;
constexpr int ADAPTER_VAL_DW = 2 * ADAPTER_QUADS + 2;
constexpr int ADAPTER_MISC_OFF = ADAPTER_SEQ_DW + ADAPTER_VAL_DW;
constexpr int ADAPTER_LDS_DW = (ADAPTER_MISC_OFF + MISC_DW + 3) & ~3;    // per wave: 124 dwords
constexpr int ADAPTER_WPG = 4;
static_assert(ADAPTER_SEQ_DW % 4 == 0 && ADAPTER_LDS_DW % 4 == 0, "seq and every wave's slice start on 16-byte boundaries (lds_store16)");
static_assert(ADAPTER_VAL_DW % 2 == 0, "the invalid words are stored 8 bytes at a time");
static_assert(ADAPTER_MAX_LEN == 64 && ADAPTER_MAX_REGION < (1 << 16), "a pattern is one 64-bit column; dist and end fit 16 bits");

// The checks of tps_batch_adapter_find (host code; the library and the emulation share them): TPS_OK, or the code and *why.
// A pattern is two uint64 of 2-bit codes (A C T G = 0 1 2 3), letter i in bits [2i, 2i + 1] of the 128, nothing behind its letters.
static inline int adapter_check(const uint64_t* patterns, const int32_t* pat_len, int n_pat, const char** why, int* at) {
    *at = 0;
    if (n_pat < 1 || n_pat > ADAPTER_MAX_PATTERNS) { *why = "n_pat must be 1..64"; return TPS_E_CAPACITY; }
    if (!patterns || !pat_len) { *why = "null patterns / pat_len"; return TPS_E_ARG; }
    for (int j = 0; j < n_pat; ++j) {
        *at = j;
        if (pat_len[j] < ADAPTER_MIN_LEN || pat_len[j] > ADAPTER_MAX_LEN) { *why = "a pattern must have 12..64 letters"; return TPS_E_CAPACITY; }
    }
    for (int j = 0; j < n_pat; ++j) {
        *at = j;
        const int m = pat_len[j];
        const uint64_t lo = patterns[2 * j], hi = patterns[2 * j + 1];
        const bool behind = m < 32 ? ((lo >> (2 * m)) != 0 || hi != 0) : m == 32 ? hi != 0 : m < 64 ? (hi >> (2 * (m - 32))) != 0 : false;
        if (behind) { *why = "a pattern has codes behind its letters"; return TPS_E_ARG; }
    }
    return TPS_OK;
}
static inline int adapter_check_reads(const uint8_t* tails, const int32_t* begin, const int32_t* end, int64_t n, const char** why, int64_t* at) {
    for (int64_t i = 0; i < n; ++i) {
        *at = i;
        if (tails[i] > 1) { *why = "tail must be 0 or 1"; return TPS_E_ARG; }
        if (begin[i] < 0 || end[i] < 0 || begin[i] > end[i]) { *why = "need 0 <= begin <= end"; return TPS_E_ARG; }
    }
    for (int64_t i = 0; i < n; ++i) {
        *at = i;
        if ((int64_t)end[i] - begin[i] > ADAPTER_MAX_REGION) { *why = "end - begin must be at most 1024"; return TPS_E_CAPACITY; }
    }
    return TPS_OK;
}
// Every refusal of tps_batch_adapter_find that needs no context, in the library's order, the message in *why (host code; the library
// and the emulation call it).  n = the reads of the batch; an empty batch needs no per-read arrays.
static inline int adapter_find_check(int64_t n, const uint64_t* patterns, const int32_t* pat_len, int n_pat, const uint8_t* tails, const int32_t* begin,
                                     const int32_t* end, int64_t n_reads, const void* hits, int64_t hits_len, Why* why) {
    const char* s = "";
    int pat_at = 0;
    int64_t at = 0;
    if (const int rc = adapter_check(patterns, pat_len, n_pat, &s, &pat_at)) return refuse(why, rc, "pattern %d: %s", pat_at, s);
    if (n_reads != n) return refuse(why, TPS_E_ARG, "tails, begin and end must hold %lld reads", (long long)n);
    if (hits_len != n * n_pat * 2) return refuse(why, TPS_E_ARG, "hits must hold %lld values", (long long)(n * n_pat * 2));
    if (n == 0) return TPS_OK;
    if (!tails || !begin || !end || !hits) return refuse(why, TPS_E_ARG, "null tails / begin / end / hits");
    if (const int rc = adapter_check_reads(tails, begin, end, n, &s, &at)) return refuse(why, rc, "read %lld: %s", (long long)at, s);
    return TPS_OK;
}
// peq[j][c]: bit i set exactly where letter i of pattern j has code c (patterns as adapter_check takes them)
static inline void adapter_build_peq(const uint64_t* patterns, const int32_t* pat_len, int n_pat, uint64_t* peq) {
    for (int j = 0; j < n_pat; ++j) {
        uint64_t* row = peq + 4 * j;
        row[0] = row[1] = row[2] = row[3] = 0;
        for (int i = 0; i < pat_len[j]; ++i) row[(patterns[2 * j + (i >> 5)] >> (2 * (i & 31))) & 3u] |= 1ull << i;
    }
}

// one step of lane j: the letter with match mask eq (0: it matches nothing) behind the column Pv / Mv; returns the change of the
// last row's score (+1, 0, -1).  Myers 1999 as restated by Hyyro: the 64-bit sum carries from bit 31 into bit 32.
TPS_DEV int adapter_step(uint64_t eq, uint64_t top, uint64_t& pv, uint64_t& mv) {
    const uint64_t xv = eq | mv;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv);
    uint64_t mh = pv & xh;
    const int d = (ph & top) ? 1 : (mh & top) ? -1 : 0;
    ph <<= 1;                                      // search form: the horizontal delta of row 0 is 0, nothing is shifted in
    mh <<= 1;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
    return d;
}

// `lds`: ADAPTER_LDS_DW dwords of the wave's own
TPS_DEV void adapter_read(const AdapterArgs& a, int64_t r, uint32_t* lds) {
    uint32_t* seq = lds;
    uint16_t* val = (uint16_t*)(lds + ADAPTER_SEQ_DW);
    uint32_t* misc = lds + ADAPTER_MISC_OFF;
    const int64_t woff = a.desc[r].word_off;
    const int64_t L = a.desc[r].len;
    const bool has_inv = (a.desc[r].flags & TPS_RD_HAS_INVALID) != 0;
    const int64_t b = a.begin[r];
    const int64_t e = (int64_t)a.end[r] < L ? (int64_t)a.end[r] : L;
    const int n = e > b ? (int)(e - b) : 0;        // letters of the region (<= ADAPTER_MAX_REGION: the host checks)
    const bool rev = a.tails[r] != 0;
    const uint32_t flip = rev ? 0xAAAAAAAAu : 0u;  // complement: A <-> T, C <-> G is code ^ 2
    const int P = a.n_pat;
    Stage st{};
    bool any_inv = false;
    if (n > 0) {
        st = stage_plan(a.seq2, a.inv, woff, L, rev, 0, b, n);
        TPS_PHASE { if (tid == 0) misc[M_INVALID] = 0; }
        TPS_SYNC();
        TPS_PHASE { stage_thread(st, has_inv, seq, val, st.nq, &misc[M_INVALID], tid); }
        TPS_SYNC();
        any_inv = has_inv && uniform(misc[M_INVALID]) != 0;
    }
    const int q0 = st.delta, q1 = st.delta + n;    // staged positions of the region: nothing at or behind q1 is consumed
    TPS_PHASE {
        if (tid < P) {
            const int m = a.pat_len[tid];
            const uint64_t p0 = a.peq[4 * tid], p1 = a.peq[4 * tid + 1], p2 = a.peq[4 * tid + 2], p3 = a.peq[4 * tid + 3];
            const uint64_t top = 1ull << (m - 1);  // (m = 64: bit 63; 1ull << m is never formed)
            uint64_t pv = ~0ull, mv = 0;
            int score = m, best = m, best_e = 0;
            for (int q = q0; q < q1;) {
                const int idx = q >> 4;
                const int stop = q1 < ((idx + 1) << 4) ? q1 : (idx + 1) << 4;
                uint32_t word = (uniform(seq[idx]) ^ flip) >> (2 * (q & 15));
                uint32_t bad = any_inv ? uniform((uint32_t)val[idx]) >> (q & 15) : 0u;
                for (; q < stop; ++q) {
                    const uint32_t c = word & 3u;
                    uint64_t eq = c == 0 ? p0 : c == 1 ? p1 : c == 2 ? p2 : p3;
                    if (bad & 1u) eq = 0;
                    word >>= 2;
                    bad >>= 1;
                    score += adapter_step(eq, top, pv, mv);
                    if (score < best) { best = score; best_e = q + 1 - q0; }
                }
            }
            a.hits[r * P + tid] = (uint32_t)best | ((uint32_t)best_e << 16);
        }
    }
}

}  // namespace tps
