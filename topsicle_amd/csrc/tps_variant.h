// tps_variant.h -- the variant census (tps_batch_variant_census): what the called telomere tract of every read is made of --
// canonical repeats of a unit U, units with one substituted letter (by place in U and letter seen), and everything else.  Written
// against tps_wave.h like motif_read (tps_motif.h): one text for gfx950 and for the host emulation (tests/emu/emu_variant.cpp), one
// 64-lane wave per read, no pattern table.
//
// The rule (exact integers; include/topsicle_hip.h states it for the caller).  h = the read (tail 0) or its reverse complement
// (tail 1), end clamped to L.  Every position i in [begin, end - m] is examined: x = h[i .. i + m) against the m rotations R_j of
// U (R_j[q] = U[(j + q) mod m]); the smallest j with Hamming(x, R_j) <= 1 decides -- distance 0 is canonical, distance 1 with the
// mismatch at q is the variant (p = (j + q) mod m, c = the letter x[q]); no such j, or a letter of x that is not ACGT, is "other".
// The position counts in bin min((end - 1 - i) / bin, n_bins - 1).
//
// How.  The tract (up to maxlengthtelo bases) is longer than the 4096 bases the staging area holds, so it is walked back from the
// boundary in pieces of `bin` positions (bin <= 4064: a piece stages bin + m - 1 <= 4095 bases), cut AT the bin edges: a piece's
// counters are one bin's, they live in LDS, and they are flushed once per piece -- into the read's totals (LDS) and into one of
// VARIANT_PARTS partial profiles in global memory (64-bit atomics; the workgroup picks the table, the host adds the tables up:
// 10 000 waves do not queue on one small table).  Tail 1 stages the REVERSED string and complements the rotations and the reported
// letter (code ^ 2) instead of the bases, as motif_read does with its unit.  A position is one lane's: the m-mer as one 32- or
// 64-bit value from the staged 2-bit codes, per rotation an XOR, the fold of every 2-bit field to one mismatch bit and a popcount;
// the rotations are wave-uniform and walked from j = m - 1 down, so that the last hit kept is the smallest j.  Canonical positions
// -- nearly all of a telomere -- are counted in a register and added once per piece; only variants take an LDS atomic each.
#pragma once
#include "tps_device.h"

namespace tps {

struct VariantArgs {
    const uint32_t* seq2;
    const uint16_t* inv;
    const tps_read_desc* desc;
    const uint8_t* tails;        // [n_reads] 0 / 1
    const int32_t* begin;        // [n_reads]
    const int32_t* end;          // [n_reads]
    uint32_t* counts;            // [n_reads][2 + 4 m], zeroed by the host
    unsigned long long* prof;    // [VARIANT_PARTS][n_bins][2 + 4 m], zeroed by the host, or nullptr
    int64_t n_reads;
    uint64_t unit;
    int32_t m, bin, n_bins;
};
constexpr int VARIANT_MAX_UNIT = 32;                       // the unit is one uint64 of 2-bit codes
constexpr int VARIANT_MIN_BIN = 64;                        // > m - 1: the piece next to the boundary holds a position
constexpr int VARIANT_MAX_BIN = FOLLOW_MAX_SPAN - VARIANT_MAX_UNIT;      // a piece stages bin + m - 1 bases
constexpr int VARIANT_MAX_BINS = 64;
constexpr int VARIANT_PARTS = 32;                          // partial profiles
constexpr int VARIANT_COLS = 2 + 4 * VARIANT_MAX_UNIT;
constexpr int VARIANT_VAL_DW = (FOLLOW_SEQ_DW / 2 + 4 + 3) & ~3;
constexpr int VARIANT_CNT_OFF = FOLLOW_SEQ_DW + VARIANT_VAL_DW;      // the piece's counters
constexpr int VARIANT_TOT_OFF = VARIANT_CNT_OFF + ((VARIANT_COLS + 3) & ~3);      // the read's
constexpr int VARIANT_MISC_OFF = VARIANT_TOT_OFF + ((VARIANT_COLS + 3) & ~3);
constexpr int VARIANT_LDS_DW = (VARIANT_MISC_OFF + MISC_DW + 3) & ~3;    // per wave
static_assert(FOLLOW_SEQ_DW % 4 == 0 && VARIANT_LDS_DW % 4 == 0, "seq and every wave's slice start on 16-byte boundaries (lds_store16)");
static_assert(VARIANT_MAX_BIN + VARIANT_MAX_UNIT - 1 < FOLLOW_MAX_SPAN, "a piece fits the staging area");
static_assert(VARIANT_MIN_BIN >= VARIANT_MAX_UNIT, "every tract of m bases or more has a position in its first piece");

// Every refusal of tps_batch_variant_census that needs no context, in the library's order (host code; the library and the emulation
// call it): TPS_OK, or the code and *why.  n = the reads of the batch.
static inline int variant_census_check(int64_t n, uint64_t unit, int m, const uint8_t* tails, const int32_t* begin, const int32_t* end, int64_t n_reads,
                                       int bin, int n_bins, const void* counts, int64_t counts_len, const void* profile, int64_t profile_len, Why* why) {
    if (m < 2 || m > VARIANT_MAX_UNIT) return refuse(why, TPS_E_ARG, "the unit must have 2..%d letters", VARIANT_MAX_UNIT);
    if (m < 32 && (unit >> (2 * m)) != 0) return refuse(why, TPS_E_ARG, "the unit has codes behind its %d letters", m);
    for (int d = 1; d < m; ++d) {
        if (m % d) continue;
        const uint64_t rot = (unit >> (2 * d)) | (unit << (2 * (m - d)));       // the unit rotated left by d letters
        if (((rot ^ unit) & (~0ull >> (64 - 2 * m))) == 0) return refuse(why, TPS_E_ARG, "the unit is a power of its first %d letters: pass the primitive root", d);
    }
    if (bin < VARIANT_MIN_BIN || bin > VARIANT_MAX_BIN) return refuse(why, TPS_E_CAPACITY, "bin must be %d..%d positions", VARIANT_MIN_BIN, VARIANT_MAX_BIN);
    if (n_bins < 1 || n_bins > VARIANT_MAX_BINS) return refuse(why, TPS_E_CAPACITY, "n_bins must be 1..%d", VARIANT_MAX_BINS);
    const int cols = 2 + 4 * m;
    if (n_reads != n) return refuse(why, TPS_E_ARG, "tails, begin and end must hold %lld reads", (long long)n);
    if (n > 0 && (!tails || !begin || !end)) return refuse(why, TPS_E_ARG, "null tails / begin / end");
    if ((!counts && n > 0) || counts_len != n * cols) return refuse(why, TPS_E_ARG, "counts must hold %lld counters", (long long)(n * cols));
    if (profile && profile_len != (int64_t)n_bins * cols) return refuse(why, TPS_E_ARG, "profile must hold %lld counters", (long long)n_bins * cols);
    for (int64_t i = 0; i < n; ++i) {
        if (tails[i] > 1) return refuse(why, TPS_E_ARG, "read %lld: tail must be 0 or 1", (long long)i);
        if (begin[i] < 0 || end[i] < 0 || begin[i] > end[i]) return refuse(why, TPS_E_ARG, "read %lld: need 0 <= begin <= end", (long long)i);
    }
    return TPS_OK;
}

TPS_DEV int variant_popc(uint32_t x) { return popc(x); }
TPS_DEV int variant_popc(uint64_t x) { return popc((uint32_t)x) + popc((uint32_t)(x >> 32)); }
TPS_DEV int variant_ctz(uint32_t x) { return __builtin_ctz(x); }
TPS_DEV int variant_ctz(uint64_t x) { return __builtin_ctzll(x); }
// one mismatch bit per letter: every 2-bit field of d folded into its low bit
TPS_DEV uint32_t variant_fold(uint32_t d) { return or_and(d, d >> 1, 0x55555555u); }
TPS_DEV uint64_t variant_fold(uint64_t d) {
    const uint64_t s = d >> 1;
    return (uint64_t)or_and((uint32_t)d, (uint32_t)s, 0x55555555u) | ((uint64_t)or_and((uint32_t)(d >> 32), (uint32_t)(s >> 32), 0x55555555u) << 32);
}

// the class of one m-mer x (letters of the staged string, not complemented) against the rotations of u (complemented with the
// string): 0 = other, 1 = canonical, 2 + 4 p + c = variant; flip = 2 where the staged string is the complement of h.
// W = uint32_t for m <= 16, uint64_t beyond.  The loop keeps the rotation's number alone (XOR, fold, popcount, compare, select per
// rotation); the mismatch of the one that decides is computed again behind it.
template <typename W>
TPS_DEV int variant_class(W x, W u, int m, uint32_t flip) {
    const W mask = (W)~(W)0 >> (8 * (int)sizeof(W) - 2 * m);
    const int top = 2 * (m - 1);
    W rj = ((W)(u << 2) | (u >> top)) & mask;          // R_(m-1); R_(j-1) = R_j moved up one letter, its last letter first
    int bj = -1;
    TPS_NOVEC
    for (int j = m - 1; j >= 0; --j) {
        if (variant_popc(variant_fold((W)(x ^ rj))) <= 1) bj = j;
        rj = ((W)(rj << 2) | (rj >> top)) & mask;
    }
    if (bj < 0) return 0;
    const W r = bj ? ((u >> (2 * bj)) | (W)(u << (2 * (m - bj)))) & mask : u;       // R_bj
    const W bmm = variant_fold((W)(x ^ r));
    if (bmm == 0) return 1;
    const int q = variant_ctz(bmm) >> 1;
    int p = bj + q;
    p = p >= m ? p - m : p;
    const uint32_t c = ((uint32_t)(x >> (2 * q)) & 3u) ^ flip;
    return 2 + 4 * p + (int)c;
}

// `part`: which partial profile this wave adds to (any value in [0, VARIANT_PARTS): the sums do not depend on it)
TPS_DEV void variant_read(const VariantArgs& a, int64_t r, uint32_t* lds, int part) {
    uint32_t* seq = lds;
    uint16_t* val = (uint16_t*)(lds + FOLLOW_SEQ_DW);
    uint32_t* cnt = lds + VARIANT_CNT_OFF;
    uint32_t* tot = lds + VARIANT_TOT_OFF;
    uint32_t* misc = lds + VARIANT_MISC_OFF;
    const int64_t woff = a.desc[r].word_off;
    const int64_t L = a.desc[r].len;
    const bool has_inv = (a.desc[r].flags & TPS_RD_HAS_INVALID) != 0;
    const int m = a.m;
    const int cols = 2 + 4 * m;
    const int64_t b = a.begin[r];
    const int64_t e = (int64_t)a.end[r] < L ? (int64_t)a.end[r] : L;
    if (e - b < m) return;                         // (the host zeroed the row)
    const bool rev = a.tails[r] != 0;
    const uint32_t flip = rev ? 2u : 0u;
    const uint64_t umask = ~0ull >> (64 - 2 * m);
    const uint64_t u = rev ? (a.unit ^ 0xAAAAAAAAAAAAAAAAull) & umask : a.unit & umask;      // complement: A <-> T, C <-> G is code ^ 2
    const uint64_t bad_bits = (1ull << m) - 1ull;
    TPS_PHASE {
        for (int c = tid; c < cols; c += NT) { cnt[c] = 0; tot[c] = 0; }
    }
    TPS_SYNC();
    for (int64_t k = 0;; ++k) {
        const int64_t top = e - k * a.bin;         // the piece: positions [lo, p1) of bin k, p1 <= top
        const int64_t lo = top - a.bin > b ? top - a.bin : b;
        const int64_t p1 = top < e - m + 1 ? top : e - m + 1;
        const int np = (int)(p1 - lo);
        if (np > 0) {
            const int bin = k < a.n_bins - 1 ? (int)k : a.n_bins - 1;
            const Stage st = stage_plan(a.seq2, a.inv, woff, L, rev, 0, lo, np + m - 1);
            TPS_PHASE { if (tid == 0) misc[M_INVALID] = 0; }
            TPS_SYNC();
            TPS_PHASE { stage_thread(st, has_inv, seq, val, st.nq + 1, &misc[M_INVALID], tid); }       // (+ a quad of zeros: v_at reads a word ahead)
            TPS_SYNC();
            const bool any_inv = has_inv && uniform(misc[M_INVALID]) != 0;
            TPS_PHASE {
                uint32_t canon = 0;
                for (int t = tid; t < np; t += NT) {
                    const int q = st.delta + t;
                    bool bad = false;
                    if (any_inv) {
                        const int idx = q >> 4;
                        const uint64_t v = (uint64_t)val[idx] | ((uint64_t)val[idx + 1] << 16) | ((uint64_t)val[idx + 2] << 32);
                        bad = ((v >> (q & 15)) & bad_bits) != 0;
                    }
                    int cls;
                    if (m <= 16) {
                        const uint32_t x = v_at(seq, q) & (uint32_t)umask;
                        cls = variant_class<uint32_t>(x, (uint32_t)u, m, flip);
                    } else {
                        const uint64_t x = ((uint64_t)v_at(seq, q) | ((uint64_t)v_at(seq, q + 16) << 32)) & umask;
                        cls = variant_class<uint64_t>(x, u, m, flip);
                    }
                    if (!bad) {
                        if (cls == 1) ++canon;
                        else if (cls > 1) lds_add(&cnt[cls], 1u);
                    }
                }
                if (canon) lds_add(&cnt[1], canon);
            }
            TPS_SYNC();
            TPS_PHASE {
                for (int c = tid; c < cols; c += NT) {
                    const uint32_t v = c == 0 ? (uint32_t)np : cnt[c];
                    if (v) {
                        tot[c] += v;
                        if (a.prof) hist_add_n(&a.prof[((int64_t)part * a.n_bins + bin) * cols + c], v);
                        cnt[c] = 0;
                    }
                }
            }
            TPS_SYNC();
        }
        if (lo == b) break;
    }
    TPS_PHASE {
        for (int c = tid; c < cols; c += NT) a.counts[r * cols + c] = tot[c];
    }
}

}  // namespace tps
