// tps_refine.h -- the boundary at base resolution and its support (tps_batch_boundary_refine): one change point per read on the
// per-position hits of the telomere repeat, by likelihood, with the evidence for it.  Written against tps_wave.h like tract_read
// (tps_tract.h), whose hit table it shares: one text for gfx950 and for the host emulation (tests/emu/emu_refine.cpp), one 64-lane
// wave per read, no pattern table.
//
// The rule (exact integers; include/topsicle_hip.h states it for the caller).  U = a primitive word of m letters, w = min(m, 8);
// h = the upper-cased read (tail 0) or its reverse complement (tail 1); the region is h[begin .. min(end, L)) and has
// N = end - begin - w + 1 positions.  x_i = 1 when h[i .. i + w) has only ACGT letters and is within Hamming distance 1 of a cyclic
// word of U.  s_i = x_i ? +hit : -miss, P(j) = the sum of s_i over begin <= i < j, j = begin .. begin + N.  pos = the smallest j with
// P(j) maximal, score = P(pos); drop = score - P(begin + N); at_score = P(at clamped to [begin, begin + N]); hits_before / hits_after
// = the x_i in front of pos and from pos on; runner = the largest P(j) over the j with |j - pos| >= sep, runner_pos = the smallest
// such j (none: 0, -1).
//
// How.  A position is one lane's work, as in the tract map: the w-letter code from the staged 2-bit words (v_at; tail 1 is staged
// reversed and the codes complemented here, code ^ 0xAAAA), one LDS read of the table's strand-0 bit, masked where a letter is not
// ACGT, one ballot B per step of 64 positions.  P needs no scan across the lanes: with `base` = P in front of the step (wave-uniform,
// carried across steps and pieces), lane t holds P(j) = base + (hit + miss) popc(B & lanes <= t) - miss (t + 1) at j = the step's
// first position + t + 1.  Every lane keeps the best (P, j) of its own positions, replaced on a strict improvement only -- its j
// ascend, so that is its smallest -- lane 0 starts from (0, begin), and one wave arg-max (max P, then min j, one 64-bit key) gives
// pos.  The first walk also leaves every step's ballot in LDS; runner comes from a second walk over the ballots alone -- no staging, no
// table -- and the counts from popcounts of masked ballots, scalar values.  The ballots are 8 bytes per step: 8 KB per wave at the
// cap of 65 536 letters, which is why the cap is there, and far less for the regions a run really has -- so the host sizes that part
// of the wave's slice by the longest region of the batch (refine_ballot_dw) and the workgroup's LDS is dynamic: 45 KB for eight waves
// at 15 000 letters, three workgroups per CU, against 96 KB and one at the cap.  The read is staged in pieces of REFINE_PIECE
// positions, a multiple of 64, so a step never straddles two pieces.
#pragma once
#include "tps_tract.h"

namespace tps {

struct RefineArgs {
    const uint32_t* seq2;
    const uint16_t* inv;
    const tps_read_desc* desc;
    const uint32_t* table;       // the hit table (tract_hit_table); the device kernel reads its copy in LDS
    const uint8_t* tails;        // [n_reads] 0 / 1
    const int32_t* begin;        // [n_reads]
    const int32_t* end;          // [n_reads]
    const int32_t* at;           // [n_reads]
    tps_refine* out;             // [n_reads], every row written whole
    int64_t n_reads;
    int32_t w, hit, miss, sep;
    int32_t bal_dw;              // dwords of ballots in a wave's slice (refine_ballot_dw)
};
constexpr int REFINE_MAX_REGION = 65536;                   // end - begin, after end is clamped to the read
constexpr int REFINE_MAX_STEPS = REFINE_MAX_REGION / NT;   // ballots kept per read
constexpr int REFINE_MAX_WEIGHT = 16, REFINE_MAX_SEP = 65535;
constexpr int REFINE_PIECE = TRACT_SPAN;                   // positions of a staged piece: 63 steps of the wave
constexpr int REFINE_NONE = -(1 << 30);                    // below every P: |P| <= 16 x 65536
constexpr int REFINE_MISC_OFF = FOLLOW_SEQ_DW + TRACT_VAL_DW;
constexpr int REFINE_KEY_OFF = (REFINE_MISC_OFF + MISC_DW + 3) & ~3;    // two 64-bit keys: the arg-max of either walk
constexpr int REFINE_BAL_OFF = REFINE_KEY_OFF + 4;
constexpr int REFINE_WPG = 8;                              // waves per workgroup: eight reads share one copy of the table
constexpr int REFINE_LDS_MAX = 160 * 1024;                 // bytes of LDS a workgroup may have on gfx950
static_assert(REFINE_PIECE % NT == 0 && REFINE_PIECE + TRACT_MAX_WORD - 1 < FOLLOW_MAX_SPAN, "a piece of whole steps fits the staging area");
static_assert(REFINE_KEY_OFF % 4 == 0 && REFINE_BAL_OFF % 4 == 0, "the keys are 8-byte aligned, every wave's slice starts on a 16-byte boundary");
static_assert((TRACT_TABLE_DW + REFINE_WPG * (REFINE_BAL_OFF + 2 * REFINE_MAX_STEPS)) * 4 <= REFINE_LDS_MAX, "a workgroup's LDS at the cap");

// dwords of a wave's slice that holds bal_dw dwords of ballots
TPS_HD int refine_lds_dw(int bal_dw) { return REFINE_BAL_OFF + bal_dw; }
// dwords of ballots the longest region of a batch needs, two per step, a multiple of 4 (host code; after boundary_refine_check)
static inline int refine_ballot_dw(int64_t n, const int64_t* offsets, const int32_t* begin, const int32_t* end, int w) {
    int64_t most = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t L = offsets[i + 1] - offsets[i];
        const int64_t npos = (end[i] < L ? end[i] : L) - begin[i] - w + 1;
        if (npos > most) most = npos;
    }
    return (int)((2 * ((most + NT - 1) / NT) + 3) & ~(int64_t)3);
}
static_assert(REFINE_MAX_WEIGHT * REFINE_MAX_REGION < -REFINE_NONE, "REFINE_NONE lies below every P");

// Every refusal of tps_batch_boundary_refine that needs no context, in the library's order, the message in *why (host code; the
// library and the emulation call it).  n = the reads of the batch, offsets[n + 1] = where they start in its bases (the lengths); an
// empty batch needs no per-read arrays.
static inline int boundary_refine_check(int64_t n, const int64_t* offsets, uint64_t unit, int m, const uint8_t* tails, const int32_t* begin, const int32_t* end,
                                        const int32_t* at, int64_t n_reads, int hit, int miss, int sep, const void* out, int64_t out_len, Why* why) {
    const char* s = "";
    if (const int rc = tract_check(unit, m, TRACT_MIN_BLOCK, 1, 0, 1, 1, &s)) return refuse(why, rc, "%s", s);
    if (hit < 1 || hit > REFINE_MAX_WEIGHT || miss < 1 || miss > REFINE_MAX_WEIGHT) return refuse(why, TPS_E_CAPACITY, "hit and miss must be 1..%d", REFINE_MAX_WEIGHT);
    if (sep < 1 || sep > REFINE_MAX_SEP) return refuse(why, TPS_E_CAPACITY, "sep must be 1..%d", REFINE_MAX_SEP);
    if (n_reads != n) return refuse(why, TPS_E_ARG, "tails, begin, end and at must hold %lld reads", (long long)n);
    if (out_len != n) return refuse(why, TPS_E_ARG, "out must hold %lld rows", (long long)n);
    if (n == 0) return TPS_OK;
    if (!tails || !begin || !end || !at || !out) return refuse(why, TPS_E_ARG, "null tails / begin / end / at / out");
    for (int64_t i = 0; i < n; ++i) {
        if (tails[i] > 1) return refuse(why, TPS_E_ARG, "read %lld: tail must be 0 or 1", (long long)i);
        if (begin[i] < 0 || end[i] < 0 || begin[i] > end[i]) return refuse(why, TPS_E_ARG, "read %lld: need 0 <= begin <= end", (long long)i);
        if (at[i] < 0) return refuse(why, TPS_E_ARG, "read %lld: at must not be negative", (long long)i);
    }
    for (int64_t i = 0; i < n; ++i) {
        const int64_t L = offsets[i + 1] - offsets[i];
        const int64_t e = end[i] < L ? end[i] : L;
        if (e - begin[i] > REFINE_MAX_REGION) return refuse(why, TPS_E_CAPACITY, "read %lld: end - begin must be at most %d", (long long)i, REFINE_MAX_REGION);
    }
    return TPS_OK;
}

// (P, j) as one key: the larger P wins, then the smaller j; 0 = nothing offered
TPS_DEV uint64_t refine_key(int32_t p, int32_t j) {
    return p == REFINE_NONE ? 0ull : ((uint64_t)(uint32_t)(p - REFINE_NONE) << 32) | (uint32_t)~(uint32_t)j;
}

// `tab`: the hit table (device: the workgroup's copy in LDS); `lds`: refine_lds_dw(a.bal_dw) dwords of the wave's own
TPS_DEV void refine_read(const RefineArgs& a, int64_t r, uint32_t* lds, const uint32_t* tab) {
    uint32_t* seq = lds;
    uint16_t* val = (uint16_t*)(lds + FOLLOW_SEQ_DW);
    uint32_t* misc = lds + REFINE_MISC_OFF;
    uint32_t* key = lds + REFINE_KEY_OFF;
    uint32_t* bal = lds + REFINE_BAL_OFF;
    const int64_t woff = a.desc[r].word_off;
    const int64_t L = a.desc[r].len;
    const bool has_inv = (a.desc[r].flags & TPS_RD_HAS_INVALID) != 0;
    const int w = a.w;
    const int64_t b = a.begin[r];
    const int64_t e = (int64_t)a.end[r] < L ? (int64_t)a.end[r] : L;
    int64_t npos = e - b - w + 1;                  // positions of the region (<= 0: none)
    if (npos > (int64_t)(a.bal_dw / 2) * NT) npos = (int64_t)(a.bal_dw / 2) * NT;      // (never: the host sized the ballots by the longest region)
    tps_refine rec;
    rec.pos = (int32_t)b; rec.score = 0; rec.drop = 0; rec.at_score = 0; rec.hits_before = 0; rec.hits_after = 0; rec.runner = 0; rec.runner_pos = -1;
    if (npos > 0) {
        const int N = (int)npos;
        const bool rev = a.tails[r] != 0;
        const uint32_t flip = rev ? 0xAAAAAAAAu : 0u;      // complement: A <-> T, C <-> G is code ^ 2
        const uint32_t cmask = (1u << (2 * w)) - 1u;
        const uint64_t bad_bits = (1ull << w) - 1ull;
        const int32_t hm = a.hit + a.miss, miss = a.miss;
        const int ln = tps_fresh_lane();
        // ---- the first walk: the hits, P at every position, every lane's best, the ballots into LDS
        Lane<int32_t> bp, bj;
        TPS_LANES { TPS_AT(bp) = tid == 0 ? 0 : REFINE_NONE; TPS_AT(bj) = (int32_t)b; }
        TPS_PHASE { if (tid < 4) key[tid] = 0; }
        int32_t base = 0;
        for (int lo = 0; lo < N; lo += REFINE_PIECE) {
            const int np = N - lo < REFINE_PIECE ? N - lo : REFINE_PIECE;
            const Stage st = stage_plan(a.seq2, a.inv, woff, L, rev, 0, b + lo, np + w - 1);
            TPS_PHASE { if (tid == 0) misc[M_INVALID] = 0; }
            TPS_SYNC();
            // (+ two quads of zeros: the lanes of the last step that lie behind the piece read there, v_at a word ahead; nq + 2 <= 67
            // quads = FOLLOW_SEQ_DW dwords)
            TPS_PHASE { stage_thread(st, has_inv, seq, val, st.nq + 2, &misc[M_INVALID], tid); }
            TPS_SYNC();
            const bool any_inv = has_inv && uniform(misc[M_INVALID]) != 0;
            const int steps = (np + NT - 1) / NT;
            const int k0 = lo / NT;
            // one step; tail: it may reach behind the piece (the last step of the last piece alone -- every other is whole, and only
            // there are the lanes' positions held against np)
            auto step = [&](int k, const bool tail) {
                Lane<bool> h;
                TPS_PHASE_WITH(ln) {
                    const int t = k * NT + tid;
                    const int q = st.delta + t;
                    const uint32_t c = (v_at(seq, q) ^ flip) & cmask;
                    uint32_t x = (tab[c >> 4] >> (2u * (c & 15u))) & 1u;
                    if (tail && t >= np) x = 0;
                    if (any_inv) {
                        const int idx = q >> 4;
                        const uint64_t v = (uint64_t)val[idx] | ((uint64_t)val[idx + 1] << 16) | ((uint64_t)val[idx + 2] << 32);
                        if (((v >> (q & 15)) & bad_bits) != 0) x = 0;
                    }
                    TPS_AT(h) = x != 0;
                }
                const uint64_t B = wave_ballot(h);
                TPS_PHASE_WITH(ln) {
                    const int t = k * NT + tid;
                    const int32_t p = base + (int32_t)mul24((uint32_t)wave_ballot_upto(B, tid), (uint32_t)hm) - miss * (tid + 1);
                    if ((!tail || t < np) && p > TPS_AT(bp)) { TPS_AT(bp) = p; TPS_AT(bj) = (int32_t)(b + lo + t + 1); }
                    if (tid == 0) {
                        u32x2 two;
                        two.x = (uint32_t)B; two.y = (uint32_t)(B >> 32);
                        lds_store8(bal + 2 * (k0 + k), two);
                    }
                }
                base += hm * (int32_t)tract_popc64(B) - miss * NT;
            };
            for (int k = 0; k < steps - 1; ++k) step(k, false);
            step(steps - 1, true);
            TPS_SYNC();                            // the next piece overwrites what this one's lanes read
        }
        TPS_PHASE { wg_max_bits(refine_key(TPS_AT(bp), TPS_AT(bj)), (uint64_t*)key); }
        TPS_SYNC();
        const int32_t score = (int32_t)uniform(key[1]) + REFINE_NONE;
        const int32_t pos = (int32_t)~uniform(key[0]);
        // ---- the second walk, over the ballots alone: the counts in front of pos and of at (scalar), the runner
        const int32_t rel = (int32_t)(pos - b);            // 0 .. N
        const int64_t at = a.at[r];
        const int32_t at_rel = at < b ? 0 : at > b + N ? N : (int32_t)(at - b);
        const int32_t sep = a.sep;
        Lane<int32_t> rp, rj;
        TPS_LANES { TPS_AT(rp) = tid == 0 && rel >= sep ? 0 : REFINE_NONE; TPS_AT(rj) = (int32_t)b; }
        // (the counts in front of rel and of at_rel: the whole steps in front of theirs, and the low bits of that one; a place at the
        // very end of whole steps has no step of its own and takes them all)
        int32_t all = 0, before = -1, before_at = -1;
        const int k_rel = rel / NT, k_at = at_rel / NT;
        base = 0;
        const int steps = (N + NT - 1) / NT;
        auto step = [&](int k, const bool tail) {
            const uint64_t B = (uint64_t)uniform(bal[2 * k]) | ((uint64_t)uniform(bal[2 * k + 1]) << 32);
            if (k == k_rel) before = all + (int32_t)tract_popc64(B & ((1ull << (rel % NT)) - 1ull));
            if (k == k_at) before_at = all + (int32_t)tract_popc64(B & ((1ull << (at_rel % NT)) - 1ull));
            const int32_t c = (int32_t)tract_popc64(B);
            all += c;
            TPS_PHASE_WITH(ln) {
                const int t = k * NT + tid;
                const int32_t p = base + (int32_t)mul24((uint32_t)wave_ballot_upto(B, tid), (uint32_t)hm) - miss * (tid + 1);
                const int32_t d = t + 1 - rel;
                if ((!tail || t < N) && (d >= sep || -d >= sep) && p > TPS_AT(rp)) { TPS_AT(rp) = p; TPS_AT(rj) = (int32_t)(b + t + 1); }
            }
            base += hm * c - miss * NT;
        };
        for (int k = 0; k < steps - 1; ++k) step(k, false);
        step(steps - 1, true);
        if (before < 0) before = all;
        if (before_at < 0) before_at = all;
        TPS_PHASE { wg_max_bits(refine_key(TPS_AT(rp), TPS_AT(rj)), (uint64_t*)(key + 2)); }
        TPS_SYNC();
        const uint32_t rk_hi = uniform(key[3]), rk_lo = uniform(key[2]);
        rec.pos = pos;
        rec.score = score;
        rec.drop = score - (hm * all - miss * N);
        rec.at_score = hm * before_at - miss * at_rel;
        rec.hits_before = before;
        rec.hits_after = all - before;
        if (rk_hi != 0) { rec.runner = (int32_t)rk_hi + REFINE_NONE; rec.runner_pos = (int32_t)~rk_lo; }
    }
    tps_refine* out = a.out + r;
    TPS_PHASE { if (tid == 0) *out = rec; }
}

}  // namespace tps
