// tps_methyl.h -- base-modification calls (BAM MM / ML tags) binned against the called boundary (tps_batch_mod_profile).  Written
// against tps_wave.h like refine_read (tps_refine.h): one text for gfx950 and for the host emulation (tests/emu/emu_methyl.cpp), one
// 64-lane wave per read, no pattern table.
//
// The rule (exact integers; include/topsicle_hip.h states it for the caller).  p = a position of the resident read, t = p (tail 0) or
// L - 1 - p (tail 1).  A position is a C when its packed code is C and its inv bit is clear, a CpG when also p + 1 < L holds a valid
// G.  Entry j of a read has the ordinal o_j = sum over i <= j of (delta_i + 1), minus 1, among the read's C's (64 bits, saturating);
// o_j >= c_total is `beyond`, otherwise the entry sits on the o_j-th C; begin <= t < end makes it in_region, there not on a CpG
// off_context, else it lands in bin floor((t - origin) / w) + nb0.  A bin takes called, the sum of the prob bytes, high (prob >= hi),
// low (prob <= lo) and, independently of the entries, cpg = the CpGs of the sequence whose t falls into it.
//
// How.  The region is the read positions [p_lo, p_hi): at most 16 384, 1 025 words of 16 bases.
//   1  The whole read's words once, a word per lane and step: the 16-bit mask of its C's, a popcount, and the popcount of the part in
//      front of p_lo -- two per-lane totals and one wave sum each at the end give c_total and rank_lo, the C's in front of the region.
//      No scan and no carry: a sum does not care about the order.
//   2  The region's words (and the one behind them, for the G after a C in bit 15) into LDS as C mask | G mask << 16, the C mask cut
//      to the region, the G mask not; beside them the exclusive running count of the region's C's per word (16 bits: <= 16 384): a
//      wave scan per 64 words and a carry.
//   3  The entries in chunks of 64: delta + 1 as a 16-bit and a 17-bit part, one wave inclusive scan each (64 x 2^17 fits 32 bits),
//      put together in 64 bits on top of the carry.  An entry whose ordinal lies in [rank_lo, rank_lo + the region's C's) finds its
//      word by binary search in the counts, its C by clearing lower set bits, tests the G bit behind it and adds to the wave's bin
//      counters in LDS.  Once the carry has passed c_total everything behind is beyond: counted, not walked.
//   4  The region's words again for cpg: C mask & (G mask >> 1 | the next word's bit 0 << 15), a bin per set bit.
//   5  Lane b writes bin b (three dwords), lanes 0 .. 7 the row.  A read with a `beyond` entry gets zero bins and MOD_BAD.
// The bin of t is (t - origin + nb0 w) / w on unsigned numbers: the host refuses a region that leaves the bins, so the sum is never
// negative and the quotient is the floor.
#pragma once
#include <stdint.h>
#include "../../include/topsicle_hip.h"
#include "tps_wave.h"
#include "tps_check.h"

namespace tps {

struct ModArgs {
    const uint32_t* seq2;
    const uint16_t* inv;
    const tps_read_desc* desc;
    const uint8_t* tails;        // [n_reads] 0 / 1
    const int32_t* begin;        // [n_reads]
    const int32_t* end;          // [n_reads]
    const int32_t* origin;       // [n_reads]
    const int64_t* mod_off;      // [n_reads + 1]: read r owns the entries mod_off[r] .. mod_off[r + 1]
    const uint32_t* delta;       // [n_mods]
    const uint8_t* prob;         // [n_mods]
    tps_mod_row* rows;           // [n_reads], every row written whole
    tps_mod_bin* bins;           // [n_reads][nb0 + nb1], every record written whole
    int64_t n_reads;
    int32_t w, nb0, nb1, hi, lo;
};
constexpr int MOD_MAX_REGION = 16384;                      // end - begin, after end is clamped to the read
constexpr int MOD_MAX_BINS = NT;                           // one lane each
constexpr int MOD_MIN_W = 16, MOD_MAX_W = 4096;
constexpr int MOD_WORDS = MOD_MAX_REGION / 16 + 2;         // a region that starts inside a word touches 1 025, + the word behind them
constexpr int MOD_CG_OFF = 0;                              // C mask | G mask << 16 per word
constexpr int MOD_CUM_OFF = (MOD_WORDS + 3) & ~3;          // the running counts, 16 bits each
constexpr int MOD_BIN_OFF = MOD_CUM_OFF + (((MOD_WORDS + 1) / 2 + 3) & ~3);   // cpg, called, high, low, sum: MOD_MAX_BINS dwords each
constexpr int MOD_LDS_DW = MOD_BIN_OFF + 5 * MOD_MAX_BINS; // per wave: 1 864 dwords
constexpr int MOD_WPG = 4;                                 // 29 KB per workgroup, five workgroups per CU
static_assert(MOD_MAX_REGION < (1 << 16), "a running count and every field of a bin fit 16 bits");
static_assert(255 * (MOD_MAX_REGION / 2) < (1ll << 32), "a bin's sum fits 32 bits");
static_assert(MOD_LDS_DW % 4 == 0 && MOD_WPG * MOD_LDS_DW * 4 <= 64 * 1024, "every wave's slice starts on a 16-byte boundary; static LDS");

// Every refusal of tps_batch_mod_profile that needs no context, in the library's order, the message in *why (host code; the library
// and the emulation call it).  n = the reads of the batch, offsets[n + 1] = where they start in its bases (the lengths); an empty
// batch needs no per-read arrays.
static inline int mod_profile_check(int64_t n, const int64_t* offsets, const uint8_t* tails, const int32_t* begin, const int32_t* end, const int32_t* origin,
                                    int64_t n_reads, const int64_t* mod_off, const uint32_t* delta, const uint8_t* prob, int64_t n_mods, int w, int nb0, int nb1,
                                    int hi, int lo, const void* rows, int64_t rows_len, const void* bins, int64_t bins_len, Why* why) {
    if (w < MOD_MIN_W || w > MOD_MAX_W) return refuse(why, TPS_E_CAPACITY, "w must be %d..%d", MOD_MIN_W, MOD_MAX_W);
    if (nb0 < 0 || nb1 < 0 || nb0 + nb1 < 1 || nb0 + nb1 > MOD_MAX_BINS) return refuse(why, TPS_E_CAPACITY, "nb0 + nb1 must be 1..%d", MOD_MAX_BINS);
    if (lo < 0 || hi > 255 || lo >= hi) return refuse(why, TPS_E_ARG, "need 0 <= lo < hi <= 255");
    if (n_reads != n) return refuse(why, TPS_E_ARG, "tails, begin, end and origin must hold %lld reads", (long long)n);
    if (rows_len != n) return refuse(why, TPS_E_ARG, "rows must hold %lld rows", (long long)n);
    if (bins_len != n * (nb0 + nb1)) return refuse(why, TPS_E_ARG, "bins must hold %lld records", (long long)(n * (nb0 + nb1)));
    if (n_mods < 0) return refuse(why, TPS_E_ARG, "n_mods must not be negative");
    if (n == 0) return TPS_OK;
    if (!tails || !begin || !end || !origin || !mod_off || !rows || !bins) return refuse(why, TPS_E_ARG, "null tails / begin / end / origin / mod_off / rows / bins");
    if (n_mods > 0 && (!delta || !prob)) return refuse(why, TPS_E_ARG, "null delta / prob");
    for (int64_t i = 0; i < n; ++i) {
        if (tails[i] > 1) return refuse(why, TPS_E_ARG, "read %lld: tail must be 0 or 1", (long long)i);
        if (begin[i] < 0 || end[i] < 0 || begin[i] > end[i]) return refuse(why, TPS_E_ARG, "read %lld: need 0 <= begin <= end", (long long)i);
        if (origin[i] < 0) return refuse(why, TPS_E_ARG, "read %lld: origin must not be negative", (long long)i);
    }
    if (mod_off[0] < 0) return refuse(why, TPS_E_ARG, "mod_off must not be negative");
    for (int64_t i = 0; i < n; ++i)
        if (mod_off[i + 1] < mod_off[i]) return refuse(why, TPS_E_ARG, "read %lld: mod_off must ascend", (long long)i);
    if (mod_off[n] != n_mods) return refuse(why, TPS_E_ARG, "mod_off must end at n_mods = %lld", (long long)n_mods);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t L = offsets[i + 1] - offsets[i];
        const int64_t b = begin[i], e = end[i] < L ? end[i] : L;
        if (e <= b) continue;
        if (e - b > MOD_MAX_REGION) return refuse(why, TPS_E_CAPACITY, "read %lld: end - begin must be at most %d", (long long)i, MOD_MAX_REGION);
        if (b < (int64_t)origin[i] - (int64_t)nb0 * w || e > (int64_t)origin[i] + (int64_t)nb1 * w)
            return refuse(why, TPS_E_ARG, "read %lld: the region leaves the bins around origin", (long long)i);
    }
    return TPS_OK;
}

// the bits 0, 2, 4 .. 30 of x as a 16-bit number
TPS_DEV uint32_t mod_even_bits(uint32_t x) {
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    return (x | (x >> 8)) & 0x0000FFFFu;
}
// a word of 16 packed bases and its invalid bits: where it holds a valid C (code 1) / a valid G (code 3), one bit per base
TPS_DEV uint32_t mod_c_mask(uint32_t v, uint32_t bad) { return mod_even_bits(v & ~(v >> 1)) & ~bad; }
TPS_DEV uint32_t mod_g_mask(uint32_t v, uint32_t bad) { return mod_even_bits(v & (v >> 1)) & ~bad; }
// the low k bits, k clamped to 0 .. 16
TPS_DEV uint32_t mod_low_bits(int64_t k) { return k <= 0 ? 0u : k >= 16 ? 0xFFFFu : (1u << (int)k) - 1u; }
// the sum of a per-lane value over the wave
TPS_DEV uint32_t mod_wave_sum(const Lane<uint32_t>& x) { return wave_read_lane(wave_incl_sum(x), NT - 1); }

constexpr uint32_t MOD_BAD = TPS_MOD_BAD;

// `lds`: MOD_LDS_DW dwords of the wave's own
TPS_DEV void mod_read(const ModArgs& a, int64_t r, uint32_t* lds) {
    uint32_t* cg = lds + MOD_CG_OFF;
    uint16_t* cum = (uint16_t*)(lds + MOD_CUM_OFF);
    uint32_t* b_cpg = lds + MOD_BIN_OFF;
    uint32_t* b_called = b_cpg + MOD_MAX_BINS;
    uint32_t* b_high = b_called + MOD_MAX_BINS;
    uint32_t* b_low = b_high + MOD_MAX_BINS;
    uint32_t* b_sum = b_low + MOD_MAX_BINS;
    const int64_t woff = a.desc[r].word_off;
    const int64_t L = a.desc[r].len;
    const bool has_inv = (a.desc[r].flags & TPS_RD_HAS_INVALID) != 0;
    const int64_t b = a.begin[r];
    const int64_t e = (int64_t)a.end[r] < L ? (int64_t)a.end[r] : L;
    const int nb = a.nb0 + a.nb1;
    uint32_t* const out_row = (uint32_t*)(a.rows + r);
    uint32_t* const out_bins = (uint32_t*)(a.bins + r * nb);
    if (e <= b) {                                  // the empty answer
        TPS_PHASE {
            if (tid < 8) out_row[tid] = 0;
            if (tid < nb) { out_bins[3 * tid] = 0; out_bins[3 * tid + 1] = 0; out_bins[3 * tid + 2] = 0; }
        }
        return;
    }
    const bool rev = a.tails[r] != 0;
    const int64_t p_lo = rev ? L - e : b, p_hi = rev ? L - b : e;      // the region in read positions
    const int64_t nwords = (L + 15) >> 4;
    const int64_t wlo = p_lo >> 4;
    const int nrw = (int)(((p_hi - 1) >> 4) - wlo) + 1;                // words of the region (<= MOD_WORDS - 1)
    const uint32_t w = (uint32_t)a.w;
    const int64_t t0 = (int64_t)a.origin[r] - (int64_t)a.nb0 * a.w;    // t of bin 0's first position (<= begin: the host checks)
    const uint32_t hi = (uint32_t)a.hi, lo = (uint32_t)a.lo;
    const int ln = tps_fresh_lane();
    // the bin of read position p (nb: it has none -- never, after the host's check)
    auto bin_of = [&](int64_t p) -> int {
        const int64_t d = (rev ? L - 1 - p : p) - t0;
        if (d < 0) return nb;
        const uint32_t q = (uint32_t)d / w;
        return q < (uint32_t)nb ? (int)q : nb;
    };
    // ---- 1: c_total, and the C's in front of the region
    Lane<uint32_t> l_tot, l_below;
    TPS_LANES { TPS_AT(l_tot) = 0; TPS_AT(l_below) = 0; }
    TPS_PHASE { for (int i = tid; i < 5 * MOD_MAX_BINS; i += NT) b_cpg[i] = 0; }
    for (int64_t w0 = 0; w0 < nwords; w0 += NT) {
        TPS_PHASE_WITH(ln) {
            const int64_t wi = w0 + tid;
            if (wi < nwords) {
                const uint32_t c = mod_c_mask(a.seq2[woff + wi], has_inv ? a.inv[woff + wi] : 0u);
                TPS_AT(l_tot) += (uint32_t)popc(c);
                TPS_AT(l_below) += (uint32_t)popc(c & mod_low_bits(p_lo - 16 * wi));
            }
        }
    }
    const uint64_t c_total = mod_wave_sum(l_tot), rank_lo = mod_wave_sum(l_below);
    // ---- 2: the region's words and their running counts into LDS
    uint32_t n_in = 0;                             // C's of the region
    for (int k0 = 0; k0 <= nrw; k0 += NT) {
        Lane<uint32_t> l_cnt;
        TPS_PHASE_WITH(ln) {
            const int k = k0 + tid;
            uint32_t c = 0, g = 0;
            if (k <= nrw) {
                const int64_t wi = wlo + k;
                if (wi < nwords) {
                    const uint32_t v = a.seq2[woff + wi], bad = has_inv ? a.inv[woff + wi] : 0u;
                    c = mod_c_mask(v, bad) & ~mod_low_bits(p_lo - 16 * wi) & mod_low_bits(p_hi - 16 * wi);
                    g = mod_g_mask(v, bad);
                }
                cg[k] = c | (g << 16);
            }
            TPS_AT(l_cnt) = (uint32_t)popc(c);
        }
        const Lane<uint32_t> l_ex = wave_excl_sum(l_cnt);
        TPS_PHASE_WITH(ln) {
            const int k = k0 + tid;
            if (k <= nrw) lds16_store(cum, (uint32_t)k, n_in + TPS_AT(l_ex));
        }
        n_in += wave_read_lane(l_ex, NT - 1) + wave_read_lane(l_cnt, NT - 1);
    }
    TPS_SYNC();
    // ---- 3: the entries
    const int64_t m0 = a.mod_off[r], m1 = a.mod_off[r + 1];
    Lane<uint32_t> l_beyond, l_inreg, l_off;
    TPS_LANES { TPS_AT(l_beyond) = 0; TPS_AT(l_inreg) = 0; TPS_AT(l_off) = 0; }
    uint64_t carry = 0;                            // the sum of delta + 1 over the entries in front of the chunk
    uint64_t beyond_rest = 0;                      // entries behind the point where the carry passed c_total
    for (int64_t j0 = m0; j0 < m1; j0 += NT) {
        if (carry >= c_total) { beyond_rest = (uint64_t)(m1 - j0); break; }
        Lane<uint32_t> l_a, l_b;
        TPS_PHASE_WITH(ln) {
            const int64_t j = j0 + tid;
            const uint64_t v = j < m1 ? (uint64_t)a.delta[j] + 1ull : 0ull;
            TPS_AT(l_a) = (uint32_t)(v & 0xFFFFu);
            TPS_AT(l_b) = (uint32_t)(v >> 16);
        }
        const Lane<uint32_t> s_a = wave_incl_sum(l_a), s_b = wave_incl_sum(l_b);
        TPS_PHASE_WITH(ln) {
            const int64_t j = j0 + tid;
            if (j < m1) {
                const uint64_t o = carry + (uint64_t)TPS_AT(s_a) + ((uint64_t)TPS_AT(s_b) << 16) - 1ull;
                if (o >= c_total) {
                    TPS_AT(l_beyond) += 1u;
                } else if (o >= rank_lo && o - rank_lo < (uint64_t)n_in) {
                    const uint32_t q = (uint32_t)(o - rank_lo);
                    int k = 0, top = nrw;          // the last word whose running count is <= q
                    while (top - k > 1) {
                        const int mid = (k + top) >> 1;
                        if (lds16_load(cum, (uint32_t)mid) <= q) k = mid; else top = mid;
                    }
                    const uint32_t u = cg[k];
                    uint32_t m = u & 0xFFFFu;
                    for (uint32_t i = q - lds16_load(cum, (uint32_t)k); i > 0 && m != 0; --i) m &= m - 1u;
                    const int bit = m != 0 ? ffs0(m) : 0;
                    const bool is_cpg = bit < 15 ? ((u >> (17 + bit)) & 1u) != 0 : ((cg[k + 1] >> 16) & 1u) != 0;
                    TPS_AT(l_inreg) += 1u;
                    const int bin = bin_of(16 * (wlo + k) + bit);
                    if (!is_cpg) {
                        TPS_AT(l_off) += 1u;
                    } else if (bin < nb) {
                        const uint32_t pr = a.prob[j];
                        lds_add(&b_called[bin], 1u);
                        lds_add(&b_sum[bin], pr);
                        if (pr >= hi) lds_add(&b_high[bin], 1u);
                        if (pr <= lo) lds_add(&b_low[bin], 1u);
                    }
                }
            }
        }
        carry += (uint64_t)wave_read_lane(s_a, NT - 1) + ((uint64_t)wave_read_lane(s_b, NT - 1) << 16);
    }
    // ---- 4: the CpGs of the sequence
    for (int k0 = 0; k0 < nrw; k0 += NT) {
        TPS_PHASE_WITH(ln) {
            const int k = k0 + tid;
            if (k < nrw) {
                const uint32_t u = cg[k];
                uint32_t m = u & ((u >> 17) | ((cg[k + 1] & 0x10000u) >> 1)) & 0xFFFFu;
                while (m != 0) {
                    const int bin = bin_of(16 * (wlo + k) + ffs0(m));
                    m &= m - 1u;
                    if (bin < nb) lds_add(&b_cpg[bin], 1u);
                }
            }
        }
    }
    TPS_SYNC();
    // ---- 5: the bins and the row
    const uint64_t n_beyond = (uint64_t)mod_wave_sum(l_beyond) + beyond_rest;
    const bool bad = n_beyond != 0;
    Lane<uint32_t> l_cpg, l_called;
    TPS_PHASE {
        uint32_t d0 = 0, d1 = 0, d2 = 0;
        TPS_AT(l_cpg) = 0; TPS_AT(l_called) = 0;
        if (tid < nb && !bad) {
            TPS_AT(l_cpg) = b_cpg[tid]; TPS_AT(l_called) = b_called[tid];
            d0 = b_cpg[tid] | (b_called[tid] << 16);
            d1 = b_high[tid] | (b_low[tid] << 16);
            d2 = b_sum[tid];
        }
        if (tid < nb) { out_bins[3 * tid] = d0; out_bins[3 * tid + 1] = d1; out_bins[3 * tid + 2] = d2; }
    }
    const uint64_t n_ent = (uint64_t)(m1 - m0);
    const uint32_t row[8] = {(uint32_t)c_total, n_ent > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n_ent, n_beyond > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n_beyond,
                             mod_wave_sum(l_inreg), mod_wave_sum(l_off), mod_wave_sum(l_cpg), mod_wave_sum(l_called), bad ? MOD_BAD : 0u};
    TPS_PHASE {
        uint32_t v = row[0];
        TPS_UNROLL
        for (int i = 1; i < 8; ++i) v = tid == i ? row[i] : v;
        if (tid < 8) out_row[tid] = v;
    }
}

}  // namespace tps
