// tps_ends.h -- end groups: a sketch of the subtelomere behind every read's called boundary (tps_batch_end_sketch) and the links
// between sketches that share enough buckets (tps_sketch_links).  Written against tps_wave.h like tract_read (tps_tract.h): one
// text for gfx950 and for the host emulation (tests/emu/emu_ends.cpp), one 64-lane wave per read / per sketch row, no pattern table.
//
// The sketch rule (exact integers; include/topsicle_hip.h states it for the caller).  h = the read (tail 0) or its reverse
// complement (tail 1), end clamped to L, w = min(m, 8).  A word h[p .. p + w) is a REPEAT WORD when it is a hit on either strand
// of tract_hit_table(unit, m).  The k-mer at i in [begin, end - k] is KEPT when its k letters are ACGT and none of its k - w + 1
// words is a repeat word; its code c = sum code(h[i + q]) << 2q, its hash x = fmix32(c ^ 0x9E3779B9), its bucket the top log2 B
// bits of x.  sketch[r][b] = the smallest hash of bucket b, 0xFFFFFFFF where there is none; kept[r] = the number of kept k-mers.
//
// How.  The window is walked in pieces of up to ENDS_PIECE k-mer positions; a piece stages np + k - 1 bases, so neighbouring
// pieces overlap by k - 1 bases and every k-mer, and every word of it, is seen whole.  Tail 1 stages the REVERSED string; its
// 2-bit codes are complemented (^ 2 per letter) before the table look-up and in c.  64 positions are one step of the wave: the
// repeat-word flags of a step are one ballot, a k-mer's k - w + 1 words are bits [tid, tid + k - w] of this step's ballot and the
// next one's (k - w <= 12), so the test is two shifts and a mask of wave-uniform values.  A letter that is not ACGT needs no
// masking of the word flags: every word of a k-mer lies inside it, and the k-mer is dropped on its own invalid bits.  The kept
// k-mers go into the wave's B buckets in LDS with one atomic minimum each -- a minimum does not depend on the order -- and the row
// leaves in one coalesced store.  The hit table is the workgroup's copy in LDS, as in the tract map.
//
// The link rule.  match(i, j) = the buckets b with s_i[b] == s_j[b] != 0xFFFFFFFF.  degree[i] = the j > i with match >= min_match;
// links[i] = the smallest max_links of them, ascending, matches[i] their match counts.
//
// How.  The sketches lie bucket-major on the device, T[b][j]: one wave per row i keeps s_i in LDS (wave-uniform values) and walks
// j = i + 1 .. n - 1 in steps of 64, one j per lane; per bucket one coalesced load of T[b][j0 ..], a compare and an add, eight
// buckets per round with their loads issued first.  The lanes at or over the threshold are one ballot; the prefix popcount of a lane's lower neighbours is its place in the row, so the
// links come out in ascending j.
#pragma once
#include "tps_tract.h"

namespace tps {

struct EndSketchArgs {
    const uint32_t* seq2;
    const uint16_t* inv;
    const tps_read_desc* desc;
    const uint32_t* table;       // tract_hit_table(unit, m); the device kernel reads its copy in LDS
    const uint8_t* tails;        // [n_reads] 0 / 1
    const int32_t* begin;        // [n_reads]
    const int32_t* end;          // [n_reads]
    uint32_t* sketch;            // [n_reads][buckets]: every entry written
    uint32_t* kept;              // [n_reads]: every entry written
    int64_t n_reads;
    int32_t w, k, buckets, shift;                  // shift = 32 - log2 buckets
};
struct LinkArgs {
    const uint32_t* t;           // [buckets][n]: the sketches, bucket-major
    int32_t* degree;             // [n]
    int32_t* links;              // [n][max_links], -1 from the host
    int32_t* matches;            // [n][max_links], 0 from the host
    int64_t n;
    int32_t buckets, min_match, max_links;
};
constexpr int ENDS_MIN_K = 8, ENDS_MAX_K = 16;             // a k-mer is one 32-bit word of 2-bit codes
constexpr int ENDS_MIN_BUCKETS = 64, ENDS_MAX_BUCKETS = 512;
constexpr int ENDS_MAX_WINDOW = 16384;                     // end - begin
constexpr uint32_t ENDS_EMPTY = 0xFFFFFFFFu;
constexpr int64_t LINKS_MAX_N = 262144;
constexpr int LINKS_MAX_LINKS = 256;
constexpr int ENDS_WPG = 8;                                // waves per workgroup: eight reads share one copy of the table
constexpr int ENDS_PIECE = FOLLOW_MAX_SPAN - 2 * NT;       // k-mer positions of a piece: 62 steps of the wave
constexpr int ENDS_VAL_DW = (FOLLOW_SEQ_DW / 2 + 4 + 3) & ~3;
constexpr int ENDS_BKT_OFF = FOLLOW_SEQ_DW + ENDS_VAL_DW;
constexpr int ENDS_MISC_OFF = ENDS_BKT_OFF + ENDS_MAX_BUCKETS;
constexpr int ENDS_LDS_DW = (ENDS_MISC_OFF + MISC_DW + 3) & ~3;         // per wave
constexpr int LINKS_WPG = 4;
constexpr int LINKS_LDS_DW = ENDS_MAX_BUCKETS;             // per wave: row i
constexpr int LINKS_UNROLL = 8;                            // buckets per round of the compare loop
static_assert(ENDS_MIN_BUCKETS % LINKS_UNROLL == 0 && LINKS_UNROLL % 4 == 0 && LINKS_LDS_DW % 4 == 0, "whole rounds, 16-byte LDS reads");
static_assert(FOLLOW_SEQ_DW % 4 == 0 && ENDS_LDS_DW % 4 == 0, "seq and every wave's slice start on 16-byte boundaries (lds_store16)");
// the step behind a piece's last one is looked up too (lanes masked): its last lane reads the word at q = 63 + ENDS_PIECE + 63
static_assert(ENDS_PIECE % NT == 0 && ((NT - 1 + ENDS_PIECE + NT - 1) >> 4) + 1 < FOLLOW_SEQ_DW, "the look-ups of a piece stay inside the staging area");
static_assert(((NT - 1 + ENDS_PIECE + ENDS_MAX_K - 1 + 63) >> 6) + 2 <= FOLLOW_SEQ_DW / 4, "a piece and its two quads of zeros fit the staging area");
static_assert(ENDS_MAX_K - TRACT_MIN_UNIT < NT, "a k-mer's words lie in two neighbouring ballots");

// MurmurHash3's 32-bit finaliser
TPS_HD uint32_t ends_fmix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

static inline int ends_log2(int b) { int l = 0; while ((1 << l) < b) ++l; return l; }

// The checks of tps_batch_end_sketch on the unit and the parameters, and on the per-read arrays (host code; the library and the
// emulation share them): TPS_OK, or the code and *why.
static inline int ends_check(uint64_t unit, int m, int k, int buckets, const char** why) {
    const int rc = tract_check(unit, m, TRACT_MIN_BLOCK, 1, 0, 1, 1, why);       // (the unit's checks; the rest of that rule at harmless values)
    if (rc) return rc;
    if (k < ENDS_MIN_K || k > ENDS_MAX_K) { *why = "k must be 8..16"; return TPS_E_CAPACITY; }
    if (buckets != 64 && buckets != 128 && buckets != 256 && buckets != 512) { *why = "buckets must be 64, 128, 256 or 512"; return TPS_E_ARG; }
    return TPS_OK;
}
static inline int ends_check_reads(const uint8_t* tails, const int32_t* begin, const int32_t* end, int64_t n, const char** why, int64_t* at) {
    for (int64_t i = 0; i < n; ++i) {
        *at = i;
        if (tails[i] > 1) { *why = "tail must be 0 or 1"; return TPS_E_ARG; }
        if (begin[i] < 0 || end[i] < 0 || begin[i] > end[i]) { *why = "need 0 <= begin <= end"; return TPS_E_ARG; }
        if ((int64_t)end[i] - begin[i] > ENDS_MAX_WINDOW) { *why = "end - begin must be at most 16384"; return TPS_E_CAPACITY; }
    }
    return TPS_OK;
}
// ... of tps_sketch_links
static inline int links_check(int64_t n, int buckets, int64_t sketch_len, int min_match, int max_links, int64_t degree_len, int64_t links_len,
                              int64_t matches_len, const char** why) {
    if (buckets != 64 && buckets != 128 && buckets != 256 && buckets != 512) { *why = "buckets must be 64, 128, 256 or 512"; return TPS_E_ARG; }
    if (n < 0 || n > LINKS_MAX_N) { *why = "n must be 0..262144"; return TPS_E_CAPACITY; }
    if (min_match < 1 || min_match > buckets) { *why = "min_match must be 1..buckets"; return TPS_E_CAPACITY; }
    if (max_links < 1 || max_links > LINKS_MAX_LINKS) { *why = "max_links must be 1..256"; return TPS_E_CAPACITY; }
    if (sketch_len != n * buckets || degree_len != n || links_len != n * max_links || matches_len != n * max_links) {
        *why = "an array length does not match n";
        return TPS_E_ARG;
    }
    return TPS_OK;
}

// Every refusal of tps_batch_end_sketch and of tps_sketch_links that needs no context, in the library's order, the message in *why
// (host code; the library and the emulation call them).  n = the reads of the batch; an empty batch needs no arrays.
static inline int end_sketch_check(int64_t n, uint64_t unit, int m, int k, int buckets, const uint8_t* tails, const int32_t* begin, const int32_t* end,
                                   int64_t n_reads, const void* sketch, int64_t sketch_len, const void* kept, int64_t kept_len, Why* why) {
    const char* s = "";
    int64_t at = 0;
    if (const int rc = ends_check(unit, m, k, buckets, &s)) return refuse(why, rc, "%s", s);
    if (n_reads != n) return refuse(why, TPS_E_ARG, "tails, begin and end must hold %lld reads", (long long)n);
    if (sketch_len != n * buckets) return refuse(why, TPS_E_ARG, "sketch must hold %lld hashes", (long long)(n * buckets));
    if (kept_len != n) return refuse(why, TPS_E_ARG, "kept must hold %lld counters", (long long)n);
    if (n == 0) return TPS_OK;
    if (!tails || !begin || !end || !sketch || !kept) return refuse(why, TPS_E_ARG, "null tails / begin / end / sketch / kept");
    if (const int rc = ends_check_reads(tails, begin, end, n, &s, &at)) return refuse(why, rc, "read %lld: %s", (long long)at, s);
    return TPS_OK;
}
static inline int sketch_links_check(const void* sketch, int64_t n, int buckets, int64_t sketch_len, int min_match, int max_links, const void* degree,
                                     int64_t degree_len, const void* links, int64_t links_len, const void* matches, int64_t matches_len, Why* why) {
    const char* s = "";
    if (const int rc = links_check(n, buckets, sketch_len, min_match, max_links, degree_len, links_len, matches_len, &s)) return refuse(why, rc, "%s", s);
    if (n > 0 && (!sketch || !degree || !links || !matches)) return refuse(why, TPS_E_ARG, "null sketch / degree / links / matches");
    return TPS_OK;
}

// the sketches bucket-major: t[b][i] = sketch[i][b] (host code, in tiles of 64 rows: both sides stay in cache)
static inline void links_transpose(const uint32_t* sketch, int64_t n, int buckets, uint32_t* t) {
    for (int64_t i0 = 0; i0 < n; i0 += 64) {
        const int64_t i1 = i0 + 64 < n ? i0 + 64 : n;
        for (int b = 0; b < buckets; ++b)
            for (int64_t i = i0; i < i1; ++i) t[(int64_t)b * n + i] = sketch[i * buckets + b];
    }
}

TPS_DEV uint32_t ends_popc64(uint64_t x) { return (uint32_t)(popc((uint32_t)x) + popc((uint32_t)(x >> 32))); }

// the repeat-word flags of step s of a staged piece: lane tid looks at the word at position s NT + tid (none at or behind nwords)
TPS_DEV uint64_t ends_word_ballot(const uint32_t* seq, const uint32_t* tab, int delta, int s, int nwords, uint32_t flip, uint32_t cmask, int ln) {
    Lane<bool> h;
    TPS_PHASE_WITH(ln) {
        const int t = s * NT + tid;
        const uint32_t c = (v_at(seq, delta + t) ^ flip) & cmask;
        const uint32_t e = (tab[c >> 4] >> (2u * (c & 15u))) & 3u;
        TPS_AT(h) = e != 0 && t < nwords;
    }
    return wave_ballot(h);
}

// is the k-mer at position t of a staged piece (q = delta + t) kept?  cur / nxt: the repeat-word ballots of t's step and of the next
// one.  (Shared with end_window_read, tps_anchor.h: the keep bits it writes are this predicate.)
TPS_DEV bool ends_keep(uint64_t cur, uint64_t nxt, uint64_t wbits, int t, int np, bool any_inv, const uint16_t* val, int q, uint64_t bad_bits, int tid) {
    const uint64_t words = ((cur >> tid) | ((nxt << 1) << (NT - 1 - tid))) & wbits;
    bool keep = t < np && words == 0;
    if (any_inv) {
        const int idx = q >> 4;
        const uint64_t v = (uint64_t)val[idx] | ((uint64_t)val[idx + 1] << 16) | ((uint64_t)val[idx + 2] << 32);
        if (((v >> (q & 15)) & bad_bits) != 0) keep = false;
    }
    return keep;
}

// `tab`: the hit table (device: the workgroup's copy in LDS)
TPS_DEV void end_sketch_read(const EndSketchArgs& a, int64_t r, uint32_t* lds, const uint32_t* tab) {
    uint32_t* seq = lds;
    uint16_t* val = (uint16_t*)(lds + FOLLOW_SEQ_DW);
    uint32_t* bkt = lds + ENDS_BKT_OFF;
    uint32_t* misc = lds + ENDS_MISC_OFF;
    const int64_t woff = a.desc[r].word_off;
    const int64_t L = a.desc[r].len;
    const bool has_inv = (a.desc[r].flags & TPS_RD_HAS_INVALID) != 0;
    const int k = a.k, w = a.w, B = a.buckets;
    const int64_t b = a.begin[r];
    const int64_t e = (int64_t)a.end[r] < L ? (int64_t)a.end[r] : L;
    const bool rev = a.tails[r] != 0;
    const uint32_t flip = rev ? 0xAAAAAAAAu : 0u;          // complement: A <-> T, C <-> G is code ^ 2
    const uint32_t cmask = (1u << (2 * w)) - 1u;
    const uint32_t kmask = 0xFFFFFFFFu >> (32 - 2 * k);
    const uint64_t bad_bits = (1ull << k) - 1ull;
    const uint64_t wbits = (1ull << (k - w + 1)) - 1ull;   // the words of one k-mer
    const int64_t npos = e - b - k + 1;                    // k-mer positions of the window (<= 0: none)
    TPS_PHASE {
        for (int c = tid; c < B; c += NT) bkt[c] = ENDS_EMPTY;
    }
    TPS_SYNC();
    uint32_t kept = 0;
    for (int64_t lo = 0; lo < npos; lo += ENDS_PIECE) {
        const int np = (int)(npos - lo < ENDS_PIECE ? npos - lo : ENDS_PIECE);
        const int nwords = np + k - w;
        const Stage st = stage_plan(a.seq2, a.inv, woff, L, rev, 0, b + lo, np + k - 1);
        TPS_PHASE { if (tid == 0) misc[M_INVALID] = 0; }
        TPS_SYNC();
        // (+ two quads of zeros: the lanes of the step behind the last one read there, v_at a word ahead)
        TPS_PHASE { stage_thread(st, has_inv, seq, val, st.nq + 2, &misc[M_INVALID], tid); }
        TPS_SYNC();
        const bool any_inv = has_inv && uniform(misc[M_INVALID]) != 0;
        const int steps = (np + NT - 1) / NT;
        const int ln = tps_fresh_lane();
        uint64_t nxt = ends_word_ballot(seq, tab, st.delta, 0, nwords, flip, cmask, ln);
        for (int s = 0; s < steps; ++s) {
            const uint64_t cur = nxt;
            nxt = ends_word_ballot(seq, tab, st.delta, s + 1, nwords, flip, cmask, ln);
            Lane<bool> kp;
            TPS_PHASE_WITH(ln) {
                const int t = s * NT + tid;
                const int q = st.delta + t;
                const bool keep = ends_keep(cur, nxt, wbits, t, np, any_inv, val, q, bad_bits, tid);
                if (keep) {
                    const uint32_t c = (v_at(seq, q) ^ flip) & kmask;
                    const uint32_t x = ends_fmix32(c ^ 0x9E3779B9u);
                    lds_min_u32(&bkt[x >> a.shift], x);
                }
                TPS_AT(kp) = keep;
            }
            kept += ends_popc64(wave_ballot(kp));
        }
        TPS_SYNC();                                // the next piece overwrites what this one's lanes read
    }
    TPS_PHASE {
        for (int c = tid; c < B; c += NT) a.sketch[r * B + c] = bkt[c];
        if (tid == 0) a.kept[r] = kept;
    }
}

// row i of the links; `row`: B dwords of the wave's LDS
TPS_DEV void sketch_links_row(const LinkArgs& a, int64_t i, uint32_t* row) {
    const int B = a.buckets;
    const int64_t n = a.n;
    TPS_PHASE {
        for (int c = tid; c < B; c += NT) row[c] = a.t[(int64_t)c * n + i];
    }
    TPS_SYNC();
    int32_t found = 0;
    const int ln = tps_fresh_lane();
    for (int64_t j0 = i + 1; j0 < n; j0 += NT) {
        Lane<uint32_t> cn;
        Lane<bool> hit;
        TPS_PHASE_WITH(ln) {
            const int64_t j = j0 + tid;
            const uint32_t* col = a.t + (j < n ? j : n - 1);      // (the lanes behind the last row load its column and are masked below)
            uint32_t c = 0;
            // eight buckets per round: their loads are issued before the first compare, so that eight are in flight per lane
            // (one bucket per round, with a branch around the empty ones: 28.8 ms at n = 20 000, a load's latency per bucket)
            for (int q = 0; q < B; q += LINKS_UNROLL) {
                uint32_t v[LINKS_UNROLL], t[LINKS_UNROLL];
                TPS_UNROLL
                for (int u = 0; u < LINKS_UNROLL; u += 4) {
                    const u32x4 x = lds_load16(row + q + u);
                    v[u] = uniform(x.x); v[u + 1] = uniform(x.y); v[u + 2] = uniform(x.z); v[u + 3] = uniform(x.w);
                }
                TPS_UNROLL
                for (int u = 0; u < LINKS_UNROLL; ++u) t[u] = col[(int64_t)(q + u) * n];
                TPS_UNROLL
                for (int u = 0; u < LINKS_UNROLL; ++u) c += (t[u] == v[u] && v[u] != ENDS_EMPTY) ? 1u : 0u;      // (an empty bucket of row i matches nothing)
            }
            TPS_AT(cn) = c;
            TPS_AT(hit) = j < n && (int32_t)c >= a.min_match;
        }
        const uint64_t bal = wave_ballot(hit);
        if (bal == 0) continue;
        if (found < a.max_links) {
            TPS_PHASE_WITH(ln) {
                const int64_t at = found + (int64_t)ends_popc64(bal & ((1ull << tid) - 1ull));
                if (TPS_AT(hit) && at < a.max_links) {
                    a.links[i * a.max_links + at] = (int32_t)(j0 + tid);
                    a.matches[i * a.max_links + at] = (int32_t)TPS_AT(cn);
                }
            }
        }
        found += (int32_t)ends_popc64(bal);
    }
    TPS_PHASE { if (tid == 0) a.degree[i] = found; }
}

}  // namespace tps
