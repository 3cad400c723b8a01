// tps_place.h -- naming end groups against a reference: n query windows placed on R reference windows (tps_window_place).  Written
// against tps_wave.h like window_offsets_row (tps_anchor.h): one text for gfx950 and for the host emulation (tests/emu/emu_place.cpp),
// one 64-lane wave per query row.
//
// The rule (exact; include/topsicle_hip.h states it for the caller).  Rows, kept positions and x = fmix32(c ^ 0x9E3779B9) as in
// tps_window_offsets.  An entry is (x, r, q) for every kept q of every reference row r; a k-mer with more than max_occ entries over
// all rows is dropped whole.  The matches of a query are the (r, q, p) with p kept in the query and (x(p), r, q) an entry.
// total[r] = the matches on r, ref = the smallest r with the largest total, runner_ref the same among the other rows.  Over the
// matches of ref, with d = q - p: the coarse bins, best, second, the fine diagonals and the lower median of tps_window_offsets.
//
// The index (place_index_build: host code, the library and the emulation share it) is built once per call and lies in global memory:
//   ent   the entries that take part, sorted by (x, r, q): r << 12 | q each;
//   keys  one pair of dwords per k-mer that takes part, sorted by x: x, and first entry | (entries - 1) << 22;
//   dir   2^bits + 1 dwords: dir[b] = the first k-mer with x >> (32 - bits) >= b (the last one: the number of k-mers).
// A look-up is dir[b] and dir[b + 1], the keys of that bucket until one is not below x (about one on average: the directory has
// between one and two buckets per k-mer), then the k-mer's entries: three dependent loads.  No wave builds or clears a table.
//
// How.  The wave's LDS holds the query's codes and keep words, total[R] and the two histograms (PLACE_LDS_DW dwords, 6.5 KB).  64
// positions are one step; a step whose 64 keep bits are clear is skipped, a lane whose bit is clear sits it out.  The query is walked
// three times with the look-ups repeated: totals, coarse votes on ref, fine votes on ref.  A lane whose k-mer has several entries
// loops over them (at most max_occ rounds; the wave leaves the loop when its last lane does).  All counting is LDS atomics; the
// maxima are wave reductions of (total << 10 | 1023 - r), the coarse and fine ends are those of window_offsets_row.
#pragma once
#include <algorithm>
#include <vector>

#include "tps_anchor.h"

namespace tps {

struct PlaceArgs {
    const uint32_t* codes;       // [n][cdw] the queries
    const uint32_t* keep;        // [n][kdw]
    const int32_t* length;       // [n]
    const uint32_t* dir;         // the index (above)
    const uint32_t* keys;
    const uint32_t* ent;
    int32_t* out;                // [PLACE_OUTS][n]: ref, total, runner_ref, runner, offset, votes, second; every entry written
    int64_t n;
    int32_t R, k, cdw, kdw, shift;       // shift = 32 - bits of the directory
};
constexpr int PLACE_MAX_REFS = 1024;
constexpr int PLACE_MAX_OCC = 64;
constexpr int PLACE_OUTS = 7;
constexpr int PLACE_MIN_BITS = 4, PLACE_MAX_BITS = 22;
constexpr int PLACE_COD_DW = ANCHOR_ROW_CDW + 4;          // (v_at reads a dword ahead)
constexpr int PLACE_KEEP_OFF = PLACE_COD_DW, PLACE_TOT_OFF = PLACE_KEEP_OFF + ANCHOR_ROW_KDW, PLACE_H_OFF = PLACE_TOT_OFF + PLACE_MAX_REFS;
constexpr int PLACE_F_OFF = PLACE_H_OFF + ANCHOR_BINS;
constexpr int PLACE_LDS_DW = PLACE_F_OFF + ANCHOR_BINS;   // per wave: 1668 dwords
// Waves per workgroup.  No wave shares anything with its neighbour; eight of them are 53 376 bytes of the static array, and three such
// groups fit the CU's 160 KiB: 6 waves per SIMD (the offsets kernel, with its table per wave: 2).
constexpr int PLACE_WPG = 8;
static_assert(PLACE_MAX_REFS * (ANCHOR_MAX_SPAN - ENDS_MIN_K + 1) < (1 << 22), "an entry's index fits 22 bits");
static_assert(PLACE_MAX_OCC <= 64 && PLACE_MAX_REFS <= 1024 && ANCHOR_MAX_SPAN * PLACE_MAX_OCC <= (1 << 18), "entries - 1 fits 6 bits, a row 10, a total 18");
static_assert(PLACE_WPG * PLACE_LDS_DW * 4 <= 65536, "a workgroup's static LDS array");

// The checks of tps_window_place (host code; the library and the emulation share them): TPS_OK, or the code and *why.
static inline int place_check(int64_t n, int64_t R, int span, int k, int max_occ, int64_t codes_len, int64_t keep_len, int64_t ref_codes_len,
                              int64_t ref_keep_len, int64_t out_len, const char** why) {
    if (k < ENDS_MIN_K || k > ENDS_MAX_K) { *why = "k must be 8..16"; return TPS_E_CAPACITY; }
    if (span < k || span > ANCHOR_MAX_SPAN) { *why = "span must be k..4096"; return TPS_E_CAPACITY; }
    if (n < 0 || n > ANCHOR_MAX_ROWS) { *why = "n must be 0..262144"; return TPS_E_CAPACITY; }
    if (R < 1 || R > PLACE_MAX_REFS) { *why = "n_ref must be 1..1024"; return TPS_E_CAPACITY; }
    if (max_occ < 1 || max_occ > PLACE_MAX_OCC) { *why = "max_occ must be 1..64"; return TPS_E_CAPACITY; }
    const int64_t cdw = (span + 15) / 16, kdw = (span + 31) / 32;
    if (codes_len != n * cdw || keep_len != n * kdw) { *why = "codes and keep must hold n rows of span letters"; return TPS_E_ARG; }
    if (ref_codes_len != R * cdw || ref_keep_len != R * kdw) { *why = "ref_codes and ref_keep must hold n_ref rows of span letters"; return TPS_E_ARG; }
    if (out_len != n) { *why = "the seven outputs must hold n entries"; return TPS_E_ARG; }
    return TPS_OK;
}
static inline int place_check_rows(const int32_t* length, int64_t n, int span, const char** why, int64_t* at) {
    for (int64_t i = 0; i < n; ++i) {
        *at = i;
        if (length[i] < 0 || length[i] > span) { *why = "length must be 0..span"; return TPS_E_ARG; }
    }
    return TPS_OK;
}

// Every refusal of tps_window_place, none of which needs the context, in the library's order, the message in *why (host code; the
// library and the emulation call it).  The reference is checked whatever n is; n = 0 needs no query arrays and no outputs.
static inline int window_place_check(const void* codes, int64_t codes_len, const void* keep, int64_t keep_len, const int32_t* length, int64_t n,
                                     const void* ref_codes, int64_t ref_codes_len, const void* ref_keep, int64_t ref_keep_len, const int32_t* ref_length,
                                     int64_t R, int span, int k, int max_occ, bool have_outs, int64_t out_len, Why* why) {
    const char* s = "";
    int64_t at = 0;
    if (const int rc = place_check(n, R, span, k, max_occ, codes_len, keep_len, ref_codes_len, ref_keep_len, out_len, &s)) return refuse(why, rc, "%s", s);
    if (!ref_codes || !ref_keep || !ref_length) return refuse(why, TPS_E_ARG, "null ref_codes / ref_keep / ref_length");
    if (const int rc = place_check_rows(ref_length, R, span, &s, &at)) return refuse(why, rc, "reference row %lld: %s", (long long)at, s);
    if (n == 0) return TPS_OK;
    if (!codes || !keep || !length || !have_outs)
        return refuse(why, TPS_E_ARG, "null codes / keep / length / ref / total / runner_ref / runner / offset / votes / second");
    if (const int rc = place_check_rows(length, n, span, &s, &at)) return refuse(why, rc, "row %lld: %s", (long long)at, s);
    return TPS_OK;
}

// The index of R reference rows (host code; the library and the emulation share it).
struct PlaceIndex {
    std::vector<uint32_t> dir, keys, ent;
    int bits = PLACE_MIN_BITS;
};
static inline void place_index_build(const uint32_t* codes, const uint32_t* keep, const int32_t* length, int R, int cdw, int kdw, int k, int max_occ,
                                     PlaceIndex& ix) {
    const uint32_t kmask = 0xFFFFFFFFu >> (32 - 2 * k);
    std::vector<uint64_t> all;                             // x << 32 | r << 12 | q: sorted, that is (x, r, q)
    for (int r = 0; r < R; ++r) {
        const uint32_t* co = codes + (int64_t)r * cdw;
        const uint32_t* kp = keep + (int64_t)r * kdw;
        for (int q = 0; q + k <= length[r]; ++q) {
            if (((kp[q >> 5] >> (q & 31)) & 1u) == 0) continue;
            const uint64_t two = ((uint64_t)((q >> 4) + 1 < cdw ? co[(q >> 4) + 1] : 0u) << 32) | co[q >> 4];
            const uint32_t x = ends_fmix32(((uint32_t)(two >> (2 * (q & 15))) & kmask) ^ 0x9E3779B9u);
            all.push_back(((uint64_t)x << 32) | ((uint64_t)r << 12) | (uint64_t)q);
        }
    }
    std::sort(all.begin(), all.end());
    ix.keys.clear();
    ix.ent.clear();
    for (size_t lo = 0, hi; lo < all.size(); lo = hi) {
        for (hi = lo + 1; hi < all.size() && (all[hi] >> 32) == (all[lo] >> 32); ++hi) {}
        if (hi - lo > (size_t)max_occ) continue;           // a repeat between ends: dropped whole
        ix.keys.push_back((uint32_t)(all[lo] >> 32));
        ix.keys.push_back((uint32_t)ix.ent.size() | ((uint32_t)(hi - lo - 1) << 22));
        for (size_t e = lo; e < hi; ++e) ix.ent.push_back((uint32_t)all[e] & 0x3FFFFFu);
    }
    const size_t U = ix.keys.size() / 2;
    ix.bits = PLACE_MIN_BITS;
    while (ix.bits < PLACE_MAX_BITS && ((size_t)1 << ix.bits) < U) ++ix.bits;
    const int shift = 32 - ix.bits;
    ix.dir.assign(((size_t)1 << ix.bits) + 2, (uint32_t)U);                             // (+ 1: the keys behind it stay 8-byte aligned)
    for (size_t j = U; j-- > 0;) ix.dir[ix.keys[2 * j] >> shift] = (uint32_t)j;          // (descending: the first k-mer of a bucket stays)
    for (size_t b = (size_t)1 << ix.bits; b-- > 0;)
        if (ix.dir[b] > ix.dir[b + 1]) ix.dir[b] = ix.dir[b + 1];                        // an empty bucket begins where the next one does
}

// the entries of the k-mer with hash x: their number (0: it takes no part) and the first one
TPS_DEV uint32_t place_lookup(const PlaceArgs& a, uint32_t x, uint32_t& first) {
    const uint32_t b = x >> a.shift;
    const uint32_t hi = a.dir[b + 1];
    for (uint32_t j = a.dir[b]; j < hi; ++j) {
        const u32x2 kv = load8((const uint8_t*)(a.keys + 2 * (size_t)j));
        if (kv.x < x) continue;
        if (kv.x != x) break;
        first = kv.y & 0x3FFFFFu;
        return (kv.y >> 22) + 1u;
    }
    return 0;
}

// One walk over the staged query.  WHAT 0: tot[r]++ for every match; 1: the coarse bin of every match on `ref`; 2: its fine
// diagonal from dlo on.
template <int WHAT>
TPS_DEV void place_walk(const PlaceArgs& a, const uint32_t* cod, const uint32_t* kp, int npos, uint32_t kmask, uint32_t* cnt, int ref, int dlo) {
    const int steps = (npos + NT - 1) / NT;
    const int ln = tps_fresh_lane();
    for (int s = 0; s < steps; ++s) {
        if (offsets_step_empty(kp, s)) continue;
        TPS_PHASE_WITH(ln) {
            const int p = s * NT + tid;
            uint32_t x, first = 0;
            const uint32_t m = offsets_kmer(cod, kp, p, npos, kmask, x) ? place_lookup(a, x, first) : 0u;
            for (uint32_t t = 0; t < m; ++t) {
                const uint32_t e = a.ent[first + t];
                const int r = (int)(e >> 12), d = (int)(e & 4095u) - p;
                if (WHAT == 0) lds_add(&cnt[r], 1u);
                else if (r == ref) {
                    if (WHAT == 1) lds_add(&cnt[(d + ANCHOR_MAX_SPAN) >> 6], 1u);
                    else if ((uint32_t)(d - dlo) < (uint32_t)ANCHOR_BINS) lds_add(&cnt[d - dlo], 1u);
                }
            }
        }
    }
}

// the smallest r != skip with the largest tot[r], as tot << 10 | 1023 - r (0: no row with a match)
TPS_DEV uint32_t place_top(const uint32_t* tot, int R, int skip) {
    Lane<uint32_t> key;
    TPS_PHASE {
        uint32_t m = 0;
        for (int r = tid; r < R; r += NT) {
            const uint32_t kc = (tot[r] << 10) | (uint32_t)(PLACE_MAX_REFS - 1 - r);
            if (r != skip && tot[r] != 0 && kc > m) m = kc;
        }
        TPS_AT(key) = m;
    }
    return wave_max_u32(key);
}

// query row i; `lds`: PLACE_LDS_DW dwords of the wave's own
TPS_DEV void window_place_row(const PlaceArgs& a, int64_t i, uint32_t* lds) {
    uint32_t* cod = lds;
    uint32_t* kp = lds + PLACE_KEEP_OFF;
    uint32_t* tot = lds + PLACE_TOT_OFF;
    uint32_t* H = lds + PLACE_H_OFF;
    uint32_t* F = lds + PLACE_F_OFF;
    const int k = a.k;
    const uint32_t kmask = 0xFFFFFFFFu >> (32 - 2 * k);
    const int npos = a.length[i] - k + 1;
    int32_t* out = a.out + i;
    int ref = -1, runner_ref = -1, best = 0;
    uint32_t total = 0, runner = 0, votes = 0, second = 0;
    if (npos > 0) {
        TPS_PHASE {
            for (int c = tid; c < PLACE_COD_DW; c += NT) cod[c] = c < a.cdw ? a.codes[i * a.cdw + c] : 0u;
            for (int c = tid; c < ANCHOR_ROW_KDW; c += NT) kp[c] = c < a.kdw ? a.keep[i * a.kdw + c] : 0u;
            for (int c = tid; c < a.R; c += NT) tot[c] = 0;
            for (int c = tid; c < 2 * ANCHOR_BINS; c += NT) H[c] = 0;      // (F lies behind H)
        }
        TPS_SYNC();
        place_walk<0>(a, cod, kp, npos, kmask, tot, 0, 0);
        TPS_SYNC();
        const uint32_t top = place_top(tot, a.R, -1);
        if (top != 0) {
            ref = PLACE_MAX_REFS - 1 - (int)(top & 1023u);
            total = top >> 10;
            const uint32_t top2 = place_top(tot, a.R, ref);
            if (top2 != 0) {
                runner_ref = PLACE_MAX_REFS - 1 - (int)(top2 & 1023u);
                runner = top2 >> 10;
            }
            place_walk<1>(a, cod, kp, npos, kmask, H, ref, 0);
            TPS_SYNC();
            offsets_best(H, best, votes, second);
            const int dlo = 64 * best - ANCHOR_MAX_SPAN;
            place_walk<2>(a, cod, kp, npos, kmask, F, ref, dlo);
            TPS_SYNC();
            offsets_median(F, votes, dlo, out + 4 * a.n);              // (total > 0: the best pair holds a vote)
        }
    }
    TPS_PHASE {
        if (tid == 0) {
            out[0] = ref;
            out[a.n] = (int32_t)total;
            out[2 * a.n] = runner_ref;
            out[3 * a.n] = (int32_t)runner;
            if (votes == 0) out[4 * a.n] = 0;
            out[5 * a.n] = (int32_t)votes;
            out[6 * a.n] = (int32_t)second;
        }
    }
}

}  // namespace tps
