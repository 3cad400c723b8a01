// tps_tract.h -- the tract map (tps_batch_tract_map): where in the WHOLE read telomere repeats lie, and on which strand.  Written
// against tps_wave.h like variant_read (tps_variant.h): one text for gfx950 and for the host emulation (tests/emu/emu_tract.cpp),
// one 64-lane wave per read, no pattern table.
//
// The rule (exact integers; include/topsicle_hip.h states it for the caller).  U = a primitive word of m letters, w = min(m, 8).
// Strand 0 is U as given, strand 1 its reverse complement; the read is taken forward, as stored.  Position i in [0, L - w] is a HIT
// on strand s when read[i .. i + w) has only ACGT letters and is within Hamming distance 1 of one of the m cyclic w-letter words of
// U_s.  Block j = positions [j block, (j + 1) block); it is FLAGGED when it holds >= min_hits hits.  A tract is a maximal run of
// flagged blocks with at most `gap` unflagged ones between neighbours, kept when it spans >= min_blocks blocks.
//
// How.  The hit set does not depend on the read: the host builds it once per call (tract_hit_table: 4^w entries of two bits, strand
// 0 and strand 1, 16 entries per dword -- 16 KB at w = 8) and the workgroup copies it into LDS.  A position is one lane's work: the
// w-letter code from the staged 2-bit words (v_at), one LDS read of the table, the two bits masked where a letter is not ACGT, two
// ballots.  64 positions are one step of the wave; a block is block / 64 steps and its count the popcounts of their ballots -- scalar
// values.  The read is staged forward in pieces of TRACT_SPAN / block whole blocks (a block never straddles two pieces), and the run
// segmentation is a wave-uniform state machine per strand that is carried across the pieces: the open tract's first block, the last
// flagged block, the hits up to it and the hits since.  A tract is closed when the next flagged block is too far away or the read
// ends, and one lane writes its record with ordinary stores.
#pragma once
#include "tps_device.h"

namespace tps {

struct TractArgs {
    const uint32_t* seq2;
    const uint16_t* inv;
    const tps_read_desc* desc;
    const uint32_t* table;       // the hit table (tract_hit_table); the device kernel reads its copy in LDS
    tps_tract* tracts;           // [n_reads][2][max_tracts], zeroed by the host
    int32_t* found;              // [n_reads][2]
    uint32_t* totals;            // [n_reads][4]: hits 0, hits 1, flagged 0, flagged 1
    int64_t n_reads;
    int32_t w, block, min_hits, gap, min_blocks, max_tracts;
};
constexpr int TRACT_MIN_UNIT = 4, TRACT_MAX_UNIT = 32;
constexpr int TRACT_MAX_WORD = 8;                          // w = min(m, 8)
constexpr int TRACT_TABLE_DW = (1 << (2 * TRACT_MAX_WORD)) / 16;        // 4^8 entries of two bits: 4096 dwords
constexpr int TRACT_MIN_BLOCK = 64, TRACT_MAX_BLOCK = 1024;             // multiples of NT
constexpr int TRACT_MAX_GAP = 64, TRACT_MAX_MIN_BLOCKS = 64, TRACT_MAX_TRACTS = 16;
constexpr int TRACT_SPAN = FOLLOW_MAX_SPAN - NT;           // positions of a piece at most; the piece itself is the multiple of `block` below it
constexpr int TRACT_WPG = 8;                               // waves per workgroup: eight reads share one copy of the table
constexpr int TRACT_VAL_DW = (FOLLOW_SEQ_DW / 2 + 4 + 3) & ~3;
constexpr int TRACT_MISC_OFF = FOLLOW_SEQ_DW + TRACT_VAL_DW;
constexpr int TRACT_LDS_DW = (TRACT_MISC_OFF + MISC_DW + 3) & ~3;       // per wave
static_assert(FOLLOW_SEQ_DW % 4 == 0 && TRACT_LDS_DW % 4 == 0 && TRACT_TABLE_DW % 4 == 0, "seq and every wave's slice start on 16-byte boundaries (lds_store16)");
static_assert(TRACT_SPAN + TRACT_MAX_WORD - 1 < FOLLOW_MAX_SPAN && TRACT_SPAN >= TRACT_MAX_BLOCK, "a piece of whole blocks fits the staging area");
static_assert(TRACT_MIN_BLOCK % NT == 0, "a step of the wave lies inside one block");

// positions of a staged piece: the largest multiple of `block` that fits
TPS_HD int tract_piece(int block) { return TRACT_SPAN / block * block; }
// dwords of the hit table for words of w letters
TPS_HD int tract_table_dw(int w) { return (1 << (2 * w)) / 16; }

// The hit table of unit (m letters, 2-bit codes, letter j in bits [2j, 2j + 1]): entry c -- the word whose letter q has code
// (c >> 2q) & 3 -- has bit s set when the word is within distance 1 of a cyclic word of U_s.  tab[tract_table_dw(w)], host code.
static inline void tract_hit_table(uint64_t unit, int m, uint32_t* tab) {
    const int w = m < TRACT_MAX_WORD ? m : TRACT_MAX_WORD;
    for (int i = 0; i < tract_table_dw(w); ++i) tab[i] = 0;
    for (int s = 0; s < 2; ++s) {
        uint32_t u[TRACT_MAX_UNIT];
        for (int j = 0; j < m; ++j)                // strand 1: the reverse complement (A <-> T, C <-> G is code ^ 2)
            u[j] = s == 0 ? (uint32_t)(unit >> (2 * j)) & 3u : ((uint32_t)(unit >> (2 * (m - 1 - j))) & 3u) ^ 2u;
        for (int j = 0; j < m; ++j) {
            uint32_t c = 0;
            for (int q = 0; q < w; ++q) c |= u[(j + q) % m] << (2 * q);
            tab[c >> 4] |= (1u << s) << (2 * (c & 15u));
            for (int q = 0; q < w; ++q)
                for (uint32_t d = 1; d < 4; ++d) {
                    const uint32_t v = c ^ (d << (2 * q));
                    tab[v >> 4] |= (1u << s) << (2 * (v & 15u));
                }
        }
    }
}

// The checks of tps_batch_tract_map on the unit and the parameters (host code; the library and the emulation share them): TPS_OK,
// or the code and *why.
static inline int tract_check(uint64_t unit, int m, int block, int min_hits, int gap, int min_blocks, int max_tracts, const char** why) {
    if (m < TRACT_MIN_UNIT || m > TRACT_MAX_UNIT) { *why = "the unit must have 4..32 letters"; return TPS_E_ARG; }
    if (m < 32 && (unit >> (2 * m)) != 0) { *why = "the unit has codes behind its letters"; return TPS_E_ARG; }
    for (int d = 1; d < m; ++d) {
        if (m % d) continue;
        const uint64_t rot = (unit >> (2 * d)) | (unit << (2 * (m - d)));       // the unit rotated left by d letters
        if (((rot ^ unit) & (~0ull >> (64 - 2 * m))) == 0) { *why = "the unit is a power of a shorter word: pass the primitive root"; return TPS_E_ARG; }
    }
    if (block < TRACT_MIN_BLOCK || block > TRACT_MAX_BLOCK || block % NT) { *why = "block must be a multiple of 64 in 64..1024"; return TPS_E_CAPACITY; }
    if (min_hits < 1 || min_hits > block) { *why = "min_hits must be 1..block"; return TPS_E_CAPACITY; }
    if (gap < 0 || gap > TRACT_MAX_GAP) { *why = "gap must be 0..64"; return TPS_E_CAPACITY; }
    if (min_blocks < 1 || min_blocks > TRACT_MAX_MIN_BLOCKS) { *why = "min_blocks must be 1..64"; return TPS_E_CAPACITY; }
    if (max_tracts < 1 || max_tracts > TRACT_MAX_TRACTS) { *why = "max_tracts must be 1..16"; return TPS_E_CAPACITY; }
    return TPS_OK;
}

// Every refusal of tps_batch_tract_map that needs no context, in the library's order, the message in *why (host code; the library and
// the emulation call it).  n = the reads of the batch; an empty batch needs no arrays.
static inline int tract_map_check(int64_t n, uint64_t unit, int m, int block, int min_hits, int gap, int min_blocks, int max_tracts, const void* tracts,
                                  int64_t tracts_len, const void* found, int64_t found_len, const void* totals, int64_t totals_len, Why* why) {
    const char* s = "";
    if (const int rc = tract_check(unit, m, block, min_hits, gap, min_blocks, max_tracts, &s)) return refuse(why, rc, "%s", s);
    if (tracts_len != n * 2 * max_tracts) return refuse(why, TPS_E_ARG, "tracts must hold %lld records", (long long)(n * 2 * max_tracts));
    if (found_len != n * 2) return refuse(why, TPS_E_ARG, "found must hold %lld counters", (long long)(n * 2));
    if (totals_len != n * 4) return refuse(why, TPS_E_ARG, "totals must hold %lld counters", (long long)(n * 4));
    if (n > 0 && (!tracts || !found || !totals)) return refuse(why, TPS_E_ARG, "null tracts / found / totals");
    return TPS_OK;
}

// one strand's run of flagged blocks (wave-uniform)
struct TractRun {
    int32_t open, first, last, found;
    uint32_t hits, pend;         // hits of [first, last]; hits of the unflagged blocks behind `last`
    uint32_t tot_hits, tot_flagged;
};

TPS_DEV void tract_close(const TractArgs& a, int64_t r, int s, int64_t L, TractRun& t) {
    const int32_t blocks = t.last + 1 - t.first;
    if (blocks >= a.min_blocks) {
        if (t.found < a.max_tracts) {
            const int64_t e = (int64_t)(t.last + 1) * a.block + a.w - 1;
            tps_tract rec;
            rec.begin = t.first * a.block;
            rec.end = (int32_t)(e < L ? e : L);
            rec.hits = (int32_t)t.hits;
            rec.blocks = blocks;
            tps_tract* out = a.tracts + ((r * 2 + s) * a.max_tracts + t.found);
            TPS_PHASE { if (tid == 0) *out = rec; }
        }
        ++t.found;
    }
    t.open = 0;
}

// block j of the read has c hits on strand s
TPS_DEV void tract_block(const TractArgs& a, int64_t r, int s, int64_t L, TractRun& t, int32_t j, uint32_t c) {
    t.tot_hits += c;
    if ((int32_t)c >= a.min_hits) {
        ++t.tot_flagged;
        if (t.open && j - t.last <= a.gap + 1) {
            t.hits += t.pend + c;
        } else {
            if (t.open) tract_close(a, r, s, L, t);
            t.open = 1;
            t.first = j;
            t.hits = c;
        }
        t.last = j;
        t.pend = 0;
    } else if (t.open) {
        t.pend += c;
    }
}

TPS_DEV uint32_t tract_popc64(uint64_t x) { return (uint32_t)(popc((uint32_t)x) + popc((uint32_t)(x >> 32))); }

// `tab`: the hit table (device: the workgroup's copy in LDS)
TPS_DEV void tract_read(const TractArgs& a, int64_t r, uint32_t* lds, const uint32_t* tab) {
    uint32_t* seq = lds;
    uint16_t* val = (uint16_t*)(lds + FOLLOW_SEQ_DW);
    uint32_t* misc = lds + TRACT_MISC_OFF;
    const int64_t woff = a.desc[r].word_off;
    const int64_t L = a.desc[r].len;
    const bool has_inv = (a.desc[r].flags & TPS_RD_HAS_INVALID) != 0;
    const int w = a.w;
    const uint32_t cmask = (1u << (2 * w)) - 1u;
    const uint64_t bad_bits = (1ull << w) - 1ull;
    const int64_t npos = L - w + 1;                // positions of the read (<= 0: none)
    const int piece = tract_piece(a.block);
    const int spb = a.block / NT;                  // steps of the wave per block
    TractRun run[2];
    for (int s = 0; s < 2; ++s) { run[s].open = 0; run[s].first = 0; run[s].last = 0; run[s].found = 0; run[s].hits = 0; run[s].pend = 0; run[s].tot_hits = 0; run[s].tot_flagged = 0; }
    int32_t j = 0;                                 // the block the next step belongs to
    for (int64_t lo = 0; lo < npos; lo += piece) {
        const int np = (int)(npos - lo < piece ? npos - lo : piece);
        const Stage st = stage_plan(a.seq2, a.inv, woff, L, false, 0, lo, np + w - 1);
        TPS_PHASE { if (tid == 0) misc[M_INVALID] = 0; }
        TPS_SYNC();
        // (+ two quads of zeros: the lanes of the last step that lie behind the piece read there, v_at a word ahead; nq + 2 <= 67
        // quads = FOLLOW_SEQ_DW dwords)
        TPS_PHASE { stage_thread(st, has_inv, seq, val, st.nq + 2, &misc[M_INVALID], tid); }
        TPS_SYNC();
        const bool any_inv = has_inv && uniform(misc[M_INVALID]) != 0;
        const int steps = (np + NT - 1) / NT;
        const int ln = tps_fresh_lane();
        uint32_t c0 = 0, c1 = 0;
        int in_block = 0;
        for (int k = 0; k < steps; ++k) {
            Lane<bool> h0, h1;
            TPS_PHASE_WITH(ln) {
                const int t = k * NT + tid;
                const int q = st.delta + t;
                const uint32_t c = v_at(seq, q) & cmask;
                uint32_t e = (tab[c >> 4] >> (2u * (c & 15u))) & 3u;
                if (t >= np) e = 0;
                if (any_inv) {
                    const int idx = q >> 4;
                    const uint64_t v = (uint64_t)val[idx] | ((uint64_t)val[idx + 1] << 16) | ((uint64_t)val[idx + 2] << 32);
                    if (((v >> (q & 15)) & bad_bits) != 0) e = 0;
                }
                TPS_AT(h0) = (e & 1u) != 0;
                TPS_AT(h1) = (e & 2u) != 0;
            }
            c0 += tract_popc64(wave_ballot(h0));
            c1 += tract_popc64(wave_ballot(h1));
            if (++in_block == spb || k == steps - 1) {      // (a piece is whole blocks: only the read's last block is short)
                tract_block(a, r, 0, L, run[0], j, c0);
                tract_block(a, r, 1, L, run[1], j, c1);
                ++j;
                c0 = c1 = 0;
                in_block = 0;
            }
        }
        TPS_SYNC();                                // the next piece overwrites what this one's lanes read
    }
    for (int s = 0; s < 2; ++s)
        if (run[s].open) tract_close(a, r, s, L, run[s]);
    TPS_PHASE {
        if (tid == 0) {
            a.found[r * 2] = run[0].found;
            a.found[r * 2 + 1] = run[1].found;
            a.totals[r * 4] = run[0].tot_hits;
            a.totals[r * 4 + 1] = run[1].tot_hits;
            a.totals[r * 4 + 2] = run[0].tot_flagged;
            a.totals[r * 4 + 3] = run[1].tot_flagged;
        }
    }
}

}  // namespace tps
