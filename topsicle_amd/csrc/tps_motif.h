// tps_motif.h -- the motif census (tps_batch_motif_census): which period repeats at a read's ends, and what the repeated word is,
// WITHOUT a pattern table.  Written against tps_wave.h like followers_wide_read (tps_wide.h): one text for gfx950 and for the host
// emulation (tests/emu/emu_motif.cpp), one 64-lane wave per read, both ends staged with stage_plan / stage_thread.
//
// The rule (exact integers; include/topsicle_hip.h states it for the caller).  h = bases [lo, min(L, hi)) of the read (end 0) or of
// its reverse complement (end 1), n = len(h).  For a period u in [u_min, u_max], w = min(u, 8):
//   eq_u[i]  = i + u < n and h[i], h[i + u] are both ACGT and equal
//   per_u[i] = eq_u[i .. i + w - 1] all set          (the w-mer at i recurs u bases on; implies i + u + w <= n)
//   C_u      = sum of per_u
// u* = the period of the largest C_u (ties: the smallest u); the run = the longest run of set per_u* (ties: the leftmost);
// unit = h[run_start .. run_start + u*).
//
// How.  Equality of bases does not care about the strand, so end 1 stages the REVERSED string and complements the unit alone
// (code ^ 2).  The staged 2-bit codes are split once per end into three bit planes with one bit per position of h -- the low
// bit of the code, the high bit, and "not a base" (the staged invalid words; every position at or past n counts as not a base,
// which is all the bounds checking the rule needs) -- so that eq_u of 32 positions is
//   ~((p0 ^ p0 >> u) | (p1 ^ p1 >> u) | bad | bad >> u)
// on 32-bit words, the shifted words being funnel shifts (v_alignbit) of two neighbours.  A work item is (period, word of 32
// positions): 39 bits of eq, the run-of-w test by shifts, a popcount added to the period's counter in LDS.  The per bitmap is then
// rebuilt for u* only; every lane takes 64 of its bits (the runs inside them, the ones at their two edges) and lane 0 joins the
// edges across lanes.
#pragma once
#include "tps_device.h"

namespace tps {

struct MotifArgs {
    const uint32_t* seq2;
    const uint16_t* inv;
    const tps_read_desc* desc;
    tps_motif_hit* hits;         // [n_reads][2], zeroed by the host
    int32_t* counts;             // [n_reads][2][u_max - u_min + 1] = C_u, zeroed by the host, or nullptr
    int64_t n_reads;
    int32_t u_min, u_max, lo, hi, min_len;
};
constexpr int MOTIF_MAX_PERIOD = 32;                       // the unit is one uint64 of 2-bit codes
constexpr int MOTIF_W = 8;                                 // letters that have to recur for a position to count
constexpr int MOTIF_PW = FOLLOW_MAX_SPAN / 32;             // words of a bitmap over the span
constexpr int MOTIF_PLANE_DW = MOTIF_PW + 4;               // + what an item reads ahead: words j + 1 (the run test) and + 2 (shifted by u <= 32)
constexpr int MOTIF_VAL_DW = (FOLLOW_SEQ_DW / 2 + 4 + 3) & ~3;
constexpr int MOTIF_P0_OFF = FOLLOW_SEQ_DW + MOTIF_VAL_DW;
constexpr int MOTIF_P1_OFF = MOTIF_P0_OFF + MOTIF_PLANE_DW;
constexpr int MOTIF_BAD_OFF = MOTIF_P1_OFF + MOTIF_PLANE_DW;
constexpr int MOTIF_PER_OFF = MOTIF_BAD_OFF + MOTIF_PLANE_DW;        // per_u* of the span
constexpr int MOTIF_CNT_OFF = MOTIF_PER_OFF + MOTIF_PW;              // C_u
constexpr int MOTIF_EDGE_OFF = MOTIF_CNT_OFF + MOTIF_MAX_PERIOD;     // the lanes' edge runs
constexpr int MOTIF_MISC_OFF = MOTIF_EDGE_OFF + NT;
constexpr int MOTIF_LDS_DW = (MOTIF_MISC_OFF + MISC_DW + 3) & ~3;    // per wave
static_assert(FOLLOW_SEQ_DW % 4 == 0 && MOTIF_LDS_DW % 4 == 0, "seq and every wave's slice start on 16-byte boundaries (lds_store16)");
static_assert(MOTIF_LDS_DW <= FOLLOW_LDS_DW, "no more LDS per wave than the followers kernel takes");
static_assert(2 * NT * 32 >= FOLLOW_MAX_SPAN, "64 bits of the per bitmap per lane cover the span");

// Every refusal of tps_batch_motif_census that needs no context, in the library's order (host code; the library and the emulation
// call it): TPS_OK, or the code and *why.  n = the reads of the batch.
static inline int motif_census_check(int64_t n, int u_min, int u_max, int lo, int hi, const void* hits, int64_t n_hits, const void* counts,
                                     int64_t counts_len, Why* why) {
    if (u_min < 1 || u_max < u_min || u_max > MOTIF_MAX_PERIOD) return refuse(why, TPS_E_ARG, "the periods must be 1 <= u_min <= u_max <= %d", MOTIF_MAX_PERIOD);
    if (lo < 0 || hi <= lo || hi - lo > FOLLOW_MAX_SPAN) return refuse(why, TPS_E_CAPACITY, "the scanned range [lo, hi) must hold 1..%d bases", FOLLOW_MAX_SPAN);
    const int nu = u_max - u_min + 1;
    if ((!hits && n > 0) || n_hits != 2 * n) return refuse(why, TPS_E_ARG, "hits must hold %lld entries", (long long)(2 * n));
    if (counts && counts_len != 2 * n * nu) return refuse(why, TPS_E_ARG, "counts must hold %lld counters", (long long)(2 * n * nu));
    return TPS_OK;
}

// the even bits of x (bit 2 j -> bit j): one plane of sixteen 2-bit codes
TPS_DEV uint32_t motif_even_bits(uint32_t x) {
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    return (x | (x >> 8)) & 0xFFFFu;
}
// eq_u of positions 32 j .. 32 j + 31
TPS_DEV uint32_t motif_eq32(const uint32_t* p0, const uint32_t* p1, const uint32_t* bad, int j, int u) {
    const int k = j + (u >> 5);
    const uint32_t sh = (uint32_t)u & 31u;
    const uint32_t d0 = p0[j] ^ alignbit(p0[k + 1], p0[k], sh);
    const uint32_t d1 = p1[j] ^ alignbit(p1[k + 1], p1[k], sh);
    return ~(d0 | d1 | bad[j] | alignbit(bad[k + 1], bad[k], sh));
}
// per_u of positions 32 j .. 32 j + 31
TPS_DEV uint32_t motif_per32(const uint32_t* p0, const uint32_t* p1, const uint32_t* bad, int j, int u) {
    const uint64_t e = (uint64_t)motif_eq32(p0, p1, bad, j, u) | ((uint64_t)motif_eq32(p0, p1, bad, j + 1, u) << 32);
    const int w = u < MOTIF_W ? u : MOTIF_W;
    uint64_t p = e;
    TPS_NOVEC
    for (int t = 1; t < w; ++t) p &= e >> t;
    return (uint32_t)p;
}
// a run of set bits as a key: the longer run wins, then the one further left (len <= 4096, start < 4096)
TPS_DEV uint32_t motif_run_key(int start, int len) { return len > 0 ? ((uint32_t)len << 12) | (uint32_t)(4095 - start) : 0u; }

TPS_DEV void motif_read(const MotifArgs& a, int64_t r, uint32_t* lds) {
    uint32_t* seq = lds;
    uint16_t* val = (uint16_t*)(lds + FOLLOW_SEQ_DW);
    uint32_t* p0 = lds + MOTIF_P0_OFF;
    uint32_t* p1 = lds + MOTIF_P1_OFF;
    uint32_t* bad = lds + MOTIF_BAD_OFF;
    uint32_t* per = lds + MOTIF_PER_OFF;
    uint32_t* cnt = lds + MOTIF_CNT_OFF;
    uint32_t* edge = lds + MOTIF_EDGE_OFF;
    uint32_t* misc = lds + MOTIF_MISC_OFF;
    const int64_t woff = a.desc[r].word_off;
    const int64_t L = a.desc[r].len;
    const bool has_inv = (a.desc[r].flags & TPS_RD_HAS_INVALID) != 0;
    if (L <= a.min_len) return;                    // (the host zeroed hits and counts)
    const int64_t m = L < a.hi ? L : a.hi;
    if (m - a.lo < (int64_t)a.u_min + (a.u_min < MOTIF_W ? a.u_min : MOTIF_W)) return;      // no period has a position to count
    const int n = (int)(m - a.lo);
    const int nu = a.u_max - a.u_min + 1;
    const int nw = (n + 31) >> 5;                  // words of a bitmap that can hold a bit
    int s = 0;                                     // an item is (period, word): word = item & (2^s - 1), 2^s >= nw
    while ((1 << s) < nw) ++s;
    for (int e = 0; e < 2; ++e) {
        const Stage st = stage_plan(a.seq2, a.inv, woff, L, e == 1, a.lo, 0, n);
        TPS_PHASE {
            if (tid == 0) misc[M_INVALID] = 0;
            if (tid < MOTIF_MAX_PERIOD) cnt[tid] = 0;
        }
        TPS_SYNC();
        TPS_PHASE { stage_thread(st, has_inv, seq, val, st.nq + 1, &misc[M_INVALID], tid); }       // (+ a quad of zeros: v_at reads a word ahead)
        TPS_SYNC();
        const bool any_inv = has_inv && uniform(misc[M_INVALID]) != 0;
        // the three planes, position i of h at bit i; words 0 .. nw + 2 are read below
        TPS_PHASE {
            for (int wd = tid; wd < nw + 3; wd += NT) {
                uint32_t b0 = 0, b1 = 0, bd = 0;
                TPS_UNROLL
                for (int hf = 0; hf < 2; ++hf) {
                    const int i0 = 32 * wd + 16 * hf;
                    uint32_t c0 = 0, c1 = 0, cb = 0xFFFFu;
                    if (i0 < n) {
                        const int q = st.delta + i0;
                        const uint32_t v = v_at(seq, q);
                        c0 = motif_even_bits(v);
                        c1 = motif_even_bits(v >> 1);
                        cb = any_inv ? ((((uint32_t)val[q >> 4] | ((uint32_t)val[(q >> 4) + 1] << 16)) >> (q & 15)) & 0xFFFFu) : 0u;
                        if (n - i0 < 16) cb |= 0xFFFFu & (0xFFFFu << (n - i0));
                    }
                    b0 |= c0 << (16 * hf);
                    b1 |= c1 << (16 * hf);
                    bd |= cb << (16 * hf);
                }
                p0[wd] = b0;
                p1[wd] = b1;
                bad[wd] = bd;
            }
        }
        TPS_SYNC();
        // C_u
        TPS_PHASE {
            for (int it = tid; it < (nu << s); it += NT) {
                const int ui = it >> s, j = it & ((1 << s) - 1);
                if (j < nw) {
                    const int c = popc(motif_per32(p0, p1, bad, j, a.u_min + ui));
                    if (c) lds_add(&cnt[ui], (uint32_t)c);
                }
            }
        }
        TPS_SYNC();
        Lane<uint32_t> ukey;                           // C_u << 6 | 63 - (u - u_min): the largest count, then the smallest period
        TPS_PHASE {
            const uint32_t c = tid < nu ? cnt[tid] : 0u;
            TPS_AT(ukey) = tid < nu ? (c << 6) | (uint32_t)(63 - tid) : 0u;
            if (a.counts && tid < nu) a.counts[(r * 2 + e) * nu + tid] = (int32_t)c;
        }
        const uint32_t ubest = wave_max_u32(ukey);
        const int support = (int)(ubest >> 6);
        if (support == 0) { TPS_SYNC(); continue; }    // (the hit stays all zeros)
        const int u = a.u_min + 63 - (int)(ubest & 63u);
        TPS_PHASE {
            for (int j = tid; j < MOTIF_PW; j += NT) per[j] = j < nw ? motif_per32(p0, p1, bad, j, u) : 0u;
        }
        TPS_SYNC();
        // the longest run: lane t holds bits 64 t .. 64 t + 63
        Lane<uint32_t> rkey;
        TPS_PHASE {
            const uint64_t x = (uint64_t)per[2 * tid] | ((uint64_t)per[2 * tid + 1] << 32);
            const int head = ~x ? __builtin_ctzll(~x) : 64;            // set bits at the low edge (64: all of them)
            const int tail = ~x ? __builtin_clzll(~x) : 64;            // ... at the high edge
            edge[tid] = (uint32_t)head | ((uint32_t)tail << 8);
            uint32_t best = 0;
            uint64_t y = x;
            int pos = 0;
            while (y) {
                const int z = __builtin_ctzll(y);
                y >>= z;
                pos += z;
                const int len = ~y ? __builtin_ctzll(~y) : 64;
                const uint32_t key = motif_run_key(64 * tid + pos, len);
                best = key > best ? key : best;
                if (len == 64) break;
                y >>= len;
                pos += len;
            }
            TPS_AT(rkey) = best;
        }
        TPS_SYNC();
        TPS_PHASE {
            if (tid == 0) {                            // runs that cross from one lane's bits into the next's
                uint32_t best = TPS_AT(rkey);
                int carry = 0;                         // set bits that end at the boundary below lane t's
                for (int t = 0; t < NT; ++t) {
                    const int head = (int)(edge[t] & 255u), tail = (int)(edge[t] >> 8);
                    const uint32_t key = motif_run_key(64 * t - carry, carry + head);
                    best = key > best ? key : best;
                    carry = head == 64 ? carry + 64 : tail;
                }
                const uint32_t last = motif_run_key(64 * NT - carry, carry);
                TPS_AT(rkey) = last > best ? last : best;
            }
        }
        const uint32_t rbest = wave_max_u32(rkey);
        TPS_PHASE {
            if (tid == 0) {
                tps_motif_hit hit;
                hit.run_len = (int32_t)(rbest >> 12);
                hit.run_start = 4095 - (int32_t)(rbest & 4095u);
                const int q = st.delta + hit.run_start;
                uint64_t unit = v_at(seq, q);
                if (u > 16) unit |= (uint64_t)v_at(seq, q + 16) << 32;
                if (e) unit ^= 0xAAAAAAAAAAAAAAAAull;              // complement: A <-> T, C <-> G is code ^ 2
                if (u < 32) unit &= (1ull << (2 * u)) - 1ull;
                hit.unit = unit;
                hit.period = u;
                hit.support = support;
                hit.n_bases = n;
                hit.reserved = 0;
                a.hits[r * 2 + e] = hit;
            }
        }
        TPS_SYNC();
    }
}

}  // namespace tps
