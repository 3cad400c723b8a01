// tps_wide.h -- the scan of WIDE pattern tables (tps_set_patterns_wide: up to 64 patterns of up to 32 letters), one kernel.
//
// The kernels of tps_device.h are built on 32-bit pattern masks and 32-bit k-mer codes; this one is not, and shares only the resident
// batch, the staging (stage_plan / stage_thread), the change point (binseg_wg) and the outputs' layout with them.  One wave owns one
// read, as there.  What differs:
//   * the code of a position is 64 bits wide: four staged dwords, three funnel shifts per 16 positions and two per position;
//   * the table is a collision-free hash of the distinct codes (host: tps_wide_plan.h): the code is folded to 32 bits
//     (lo + rotate(hi): an XOR would send every homopolymer of 32 letters to 0), ONE 32-bit multiply picks one of 256 slots, one
//     16-byte LDS read gives (key lo, key hi, group + 1), the whole key is compared.  An unused slot holds group + 1 = 0: no code is reserved as a marker (all ones IS a code at k = 32);
//   * a position holds at most one distinct k-mer, so the table yields a GROUP id (the distinct codes, numbered with the
//     self-overlapping ones first), not a mask; one byte per position (group + 1, 0 = nothing) is what the counting phases read.
//     Duplicates of the list are a group -> patterns map (pg[]) applied when counts leave;
//   * windows are counted by LANES: a lane takes m consecutive windows of the tile, counts the first one position by position and
//     then SLIDES -- the positions that leave are taken off, the ones that enter are added (2 x slide byte reads per window instead
//     of W - k), the counts of the lane's current window live in 64 private LDS bytes.  S_w = sum of max(1, count) is kept as a
//     running value: an occurrence that makes a count 2 or more adds the group's number of list patterns, one that leaves a count
//     of 1 or more takes it off.  That is exact for every k-mer without a period (two occurrences cannot overlap).  Only groups
//     WITH a period (homopolymers, ACAC...) are walked leftmost-first per window, and only in windows that hold one of them;
//   * raw rows leave through the whole wave: after every step the 64 lanes hold one finished window each, and lane (window, pattern)
//     stores one byte -- a row is one contiguous piece of HBM;
//   * the change point is binseg_wg on the stored sums, in the same launch (the standalone kernel's arithmetic, TPS_RES_TIE alike).
//
// Written against tps_wave.h like tps_device.h: the same text compiles under TPS_EMU (tests/emu/emu_wide.cpp).
#pragma once
#include "tps_device.h"

namespace tps {

constexpr int WIDE_SLOTS = 256;                       // hash slots of 16 bytes: 4 KB per workgroup
constexpr int WIDE_TAB_DW = 4 * WIDE_SLOTS;
constexpr int WIDE_GM_DW = 64;                        // per group: how many list patterns spell it
constexpr int WIDE_PG_DW = 16;                        // per list pattern: its group (bytes)
constexpr int WIDE_IMG_DW = WIDE_TAB_DW + WIDE_GM_DW + WIDE_PG_DW;
constexpr int WIDE_CS = 17;                           // dwords of a lane's 64 byte counters (+ 1: the lanes' rows start on different banks)
constexpr int WIDE_CNT_DW = NT * WIDE_CS;             // also step 1's histogram and the change point's scratch
constexpr int WIDE_TP_MIN = 4096;                     // positions a tile holds at least
constexpr int WIDE_TP_MAX = 32768;                    // ... and at most (a window or step-1 head longer than that is refused)

struct WidePat {
    int32_t P, k;
    int32_t n_groups;        // distinct k-mers of the list
    int32_t n_so;            // groups 0 .. n_so - 1 can overlap themselves (have a period < k)
    uint32_t mask_lo, mask_hi;   // the low 2k bits
    uint32_t rot, mul;       // slot = ((lo + rotate_right(hi, rot)) * mul) >> 24
};

struct WideArgs {
    const uint32_t* seq2;        // the resident packed batch, as in ScanArgs
    const uint16_t* inv;
    const tps_read_desc* desc;
    const uint8_t* tails_in;     // n, or nullptr
    const uint32_t* img;         // WIDE_IMG_DW dwords: hash table, group multiplicities, pattern -> group
    tps_read_result* results;
    int32_t* c_start;            // n * P or nullptr
    int32_t* c_end;
    const int64_t* win_off;      // n + 1
    int32_t* sums;               // int32 at win_off[r] (whenever the window step runs)
    uint8_t* raw;                // u8 at win_off[r] * P, or nullptr
    const int32_t* order;        // n, or nullptr (plan_dispatch_order)
    int64_t n_reads;
    WidePat pat;
    tps_params prm;
    int32_t tp_cap;              // positions a tile can hold
    int32_t tw;                  // windows per tile
    int32_t seq_dw;              // dwords of the staged bases
    int32_t wpg;                 // waves per workgroup
};

TPS_HD int64_t wide_nx_dw(const WideArgs& a) { return ((int64_t)NT * a.pat.n_so + 1) / 2; }
TPS_HD int64_t wide_lds_dwords(const WideArgs& a) {          // per wave
    const int64_t dw = WIDE_CNT_DW + 2 * NT + a.seq_dw + (a.seq_dw / 2 + 4) + (a.tp_cap / 4 + 8) + wide_nx_dw(a) + MISC_DW;
    return (dw + 3) & ~3ll;
}
TPS_HD int64_t wide_wg_lds_dwords(const WideArgs& a) { return WIDE_IMG_DW + (int64_t)a.wpg * wide_lds_dwords(a); }

struct WideLds {
    uint32_t* cnt;       // NT x WIDE_CS: the lanes' byte counters
    uint32_t* st;        // 2 NT: a lane's running S_w and its count of self-overlapping occurrences in the window
    uint32_t* seq;
    uint16_t* val;
    uint32_t* pm;        // one byte per position: group + 1
    uint16_t* nx;        // NT x n_so: the walk's next admissible start per self-overlapping group
    uint32_t* misc;
    const uint32_t* tab;
    const uint32_t* gm;
    const uint8_t* pg;
};
TPS_DEV WideLds wide_carve(uint32_t* base, const uint32_t* img, const WideArgs& a) {
    WideLds l;
    uint32_t* p = base;
    l.cnt = p;  p += WIDE_CNT_DW;
    l.st = p;   p += 2 * NT;
    l.seq = p;  p += a.seq_dw;
    l.val = (uint16_t*)p;  p += a.seq_dw / 2 + 4;
    l.pm = p;   p += a.tp_cap / 4 + 8;
    l.nx = (uint16_t*)p;   p += wide_nx_dw(a);
    l.misc = p;
    l.tab = img;
    l.gm = img + WIDE_TAB_DW;
    l.pg = (const uint8_t*)(img + WIDE_TAB_DW + WIDE_GM_DW);
    return l;
}

// group + 1 of the k-mer whose code is the low 2k bits of hi:lo, 0 if the list does not hold it
TPS_DEV uint32_t wide_gid1(const WidePat& pat, const uint32_t* tab, uint32_t lo, uint32_t hi) {
    lo &= pat.mask_lo;
    hi &= pat.mask_hi;
    const uint32_t f = lo + alignbit(hi, hi, pat.rot);
    const uint32_t slot = (f * pat.mul) >> 24;
    const u32x4 e = lds_load16(tab + 4 * slot);
    return (e.x == lo && e.y == hi) ? e.z : 0u;          // (an unused slot: key 0, group + 1 = 0)
}

// pm[p] = group + 1 of the k-mer at start position p of the staged range, p < npos; lane `tid` takes chunks of 16 positions
TPS_DEV void wide_lookup(const WideArgs& a, const WideLds& l, int delta, int npos, bool inv, int tid) {
    const int nch = (npos + 15) >> 4;
    for (int c = tid; c < nch; c += NT) {
        const int p0 = c * 16, q0 = delta + p0, idx = q0 >> 4;
        const uint32_t sh = (uint32_t)(q0 & 15) * 2u;
        const uint32_t d0 = l.seq[idx], d1 = l.seq[idx + 1], d2 = l.seq[idx + 2], d3 = l.seq[idx + 3];
        const uint32_t w0 = alignbit(d1, d0, sh), w1 = alignbit(d2, d1, sh), w2 = alignbit(d3, d2, sh);
        uint32_t out[4];
        TPS_UNROLL
        for (int g4 = 0; g4 < 4; ++g4) {
            uint32_t pk = 0;
            TPS_UNROLL
            for (int i = 0; i < 4; ++i) {
                const int j = 4 * g4 + i;
                const uint32_t lo = j ? alignbit(w1, w0, 2u * j) : w0;
                const uint32_t hi = j ? alignbit(w2, w1, 2u * j) : w1;
                uint32_t g1 = wide_gid1(a.pat, l.tab, lo, hi);
                if (p0 + j >= npos) g1 = 0;
                if (inv && g1 && invalid_at(l.val, q0 + j, a.pat.k)) g1 = 0;
                pk |= g1 << (8 * i);
            }
            out[g4] = pk;
        }
        u32x4 o;
        o.x = out[0]; o.y = out[1]; o.z = out[2]; o.w = out[3];
        lds_store16(l.pm + 4 * c, o);
    }
}

// stage s-indices [i0, i0 + n) of a tail and look every start position up; returns npos.  Called by the whole wave.
TPS_DEV int wide_stage_lookup(const WideArgs& a, const WideLds& l, int64_t woff, int64_t L, bool reverse, int64_t t, int64_t i0, int n, bool has_inv) {
    const Stage st = stage_plan(a.seq2, a.inv, woff, L, reverse, t, i0, n);
    const int nqd = st.nq + 1;                             // (+ a quad of zeros: the last chunk reads three dwords ahead)
    TPS_PHASE { if (tid == 0) l.misc[M_INVALID] = 0; }
    TPS_SYNC();
    TPS_PHASE { stage_thread(st, has_inv, l.seq, l.val, nqd, &l.misc[M_INVALID], tid); }
    TPS_SYNC();
    const bool inv = has_inv && uniform(l.misc[M_INVALID]) != 0;
    const int npos = n - a.pat.k + 1 > 0 ? n - a.pat.k + 1 : 0;
    TPS_PHASE { wide_lookup(a, l, st.delta, npos, inv, tid); }
    TPS_SYNC();
    return npos;
}

// step 1 of one side: per-pattern counts of the head -> c_out[P] (or nullptr), the first maximum as count << 6 | 63 - pattern
TPS_DEV uint32_t wide_trc_side(const WideArgs& a, const WideLds& l, int64_t woff, int64_t L, bool reverse, int n1, bool has_inv, int32_t* c_out, int side) {
    const WidePat& pat = a.pat;
    TPS_PHASE { l.cnt[tid] = 0; }
    const int npos = wide_stage_lookup(a, l, woff, L, reverse, 0, 0, n1, has_inv);
    TPS_PHASE {
        const int nch = (npos + 15) >> 4;
        for (int c = tid; c < nch; c += NT) {
            const u32x4 v = lds_load16(l.pm + 4 * c);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            TPS_UNROLL
            for (int j = 0; j < 16; ++j) {
                const uint32_t g1 = (w[j >> 2] >> (8 * (j & 3))) & 255u;
                if (g1 > (uint32_t)pat.n_so) lds_add(&l.cnt[g1 - 1], 1u);     // a k-mer without a period: its occurrences cannot overlap
            }
        }
    }
    TPS_SYNC();
    if (pat.n_so) {
        // a k-mer with a period: leftmost non-overlapping, one lane per such group
        TPS_PHASE {
            if (tid < pat.n_so) {
                const uint8_t* pmb = (const uint8_t*)l.pm;
                uint32_t cnt = 0;
                int next = 0;
                for (int p = 0; p < npos; ++p)
                    if (pmb[p] == (uint8_t)(tid + 1) && p >= next) { ++cnt; next = p + pat.k; }
                l.cnt[tid] = cnt;
            }
        }
        TPS_SYNC();
    }
    TPS_PHASE {
        if (tid < pat.P) {
            const uint32_t c = l.cnt[l.pg[tid]];
            if (c_out) g32_store((uint64_t)(uintptr_t)c_out, (uint32_t)tid, c);
            lds_max_i32((int32_t*)&l.misc[M_BEST + side], (int32_t)((c << 6) | (uint32_t)(63 - tid)));
        }
    }
    TPS_SYNC();
    return uniform(l.misc[M_BEST + side]);
}

// an occurrence (g1 = group + 1 of its position, 0 = none) enters / leaves a lane's window: the group's byte counter, the running
// S_w = sum of max(1, count) over the list patterns, and the number of self-overlapping occurrences in the window (walked, not slid)
// (S and nso change by VALUES computed on both paths: written as `if (...) ++nso; else S += ...` the compiler stores through a selected
// pointer and both live in scratch)
TPS_DEV void wide_enter(const WideLds& l, const WidePat& pat, uint8_t* cb, uint32_t g1, uint32_t& S, uint32_t& nso) {
    const bool so = g1 != 0 && g1 <= (uint32_t)pat.n_so;
    uint32_t ds = 0;
    if (g1 != 0 && !so) {
        const uint32_t c = cb[g1 - 1];
        cb[g1 - 1] = (uint8_t)(c + 1);
        ds = c >= 1 ? l.gm[g1 - 1] : 0u;
    }
    S += ds;
    nso += so ? 1u : 0u;
}
TPS_DEV void wide_leave(const WideLds& l, const WidePat& pat, uint8_t* cb, uint32_t g1, uint32_t& S, uint32_t& nso) {
    const bool so = g1 != 0 && g1 <= (uint32_t)pat.n_so;
    uint32_t ds = 0;
    if (g1 != 0 && !so) {
        const uint32_t c = cb[g1 - 1];
        cb[g1 - 1] = (uint8_t)(c - 1);
        ds = c >= 2 ? l.gm[g1 - 1] : 0u;
    }
    S -= ds;
    nso -= so ? 1u : 0u;
}

// one step of the window phase: lane `tid` brings its counters to window wl = tid * m + j of the tile and stores that window's S_w
TPS_DEV void wide_step(const WideArgs& a, const WideLds& l, int j, int m, int nw_tile, int lw1, uint64_t sums_g, int tid) {
    const int wl = tid * m + j;
    if (wl >= nw_tile) return;
    const WidePat& pat = a.pat;
    const int s = a.prm.slide;
    uint8_t* cb = (uint8_t*)(l.cnt + tid * WIDE_CS);
    const uint8_t* pmb = (const uint8_t*)l.pm;
    uint32_t S, nso;
    const int base = wl * s;
    if (j == 0) {
        for (int i = 0; i < WIDE_CS; ++i) l.cnt[tid * WIDE_CS + i] = 0;
        S = (uint32_t)pat.P;                               // every pattern absent: each counts as 1
        nso = 0;
        for (int p = base; p < base + lw1; ++p) wide_enter(l, pat, cb, pmb[p], S, nso);
    } else {
        S = l.st[tid];
        nso = l.st[NT + tid];
        const int prev = base - s;
        const int gone = prev + (s < lw1 ? s : lw1);
        for (int p = prev; p < gone; ++p) wide_leave(l, pat, cb, pmb[p], S, nso);
        for (int p = (base > prev + lw1 ? base : prev + lw1); p < base + lw1; ++p) wide_enter(l, pat, cb, pmb[p], S, nso);
    }
    uint32_t extra = 0;
    if (pat.n_so) {
        uint16_t* nx = l.nx + tid * pat.n_so;
        for (int i = 0; i < pat.n_so; ++i) { cb[i] = 0; nx[i] = 0; }
        if (nso) {
            for (int p = base; p < base + lw1; ++p) {
                const uint32_t g1 = pmb[p];
                if (g1 && g1 <= (uint32_t)pat.n_so && p >= (int)nx[g1 - 1]) {
                    const uint32_t c = cb[g1 - 1];
                    cb[g1 - 1] = (uint8_t)(c + 1);
                    nx[g1 - 1] = (uint16_t)(p + pat.k);
                    if (c >= 1) extra += l.gm[g1 - 1];
                }
            }
        }
    }
    l.st[tid] = S;
    l.st[NT + tid] = nso;
    g32_store(sums_g, (uint32_t)wl, S + extra);
}

// the raw rows of the 64 windows the lanes have just finished: lane (window, pattern) stores max(1, count)
TPS_DEV void wide_rows(const WideArgs& a, const WideLds& l, int j, int m, int nw_tile, uint64_t raw_g, int tid) {
    const int P = a.pat.P;
    const int wpi = NT / P;                                // windows per store instruction
    const int sub = tid / P, p = tid - sub * P;
    if (sub >= wpi) return;
    const uint32_t g = l.pg[p];
    for (int lw = sub; lw < NT && lw * m + j < nw_tile; lw += wpi) {
        const uint32_t c = ((const uint8_t*)(l.cnt + lw * WIDE_CS))[g];
        g8_store(raw_g, (uint32_t)((lw * m + j) * P + p), c ? c : 1u);
    }
}

// ------------------------------------------------------------------ the per-read program
// `lds_base` is this wave's LDS slice, `img` the workgroup's copy of WideArgs::img.  Every lane of the wave executes this.
TPS_DEV void wide_read(const WideArgs& a, int64_t r, uint32_t* lds_base, const uint32_t* img) {
    const WideLds l = wide_carve(lds_base, img, a);
    const WidePat& pat = a.pat;
    const tps_params& prm = a.prm;
    const int64_t woff = a.desc[r].word_off;
    const int64_t L = a.desc[r].len;
    const bool has_inv = (a.desc[r].flags & TPS_RD_HAS_INVALID) != 0;
    const bool step1 = (prm.flags & TPS_F_STEP1) != 0;

    TPS_PHASE { for (int i = tid; i < MISC_DW; i += NT) l.misc[i] = 0; }
    TPS_SYNC();

    int tail = 0, pass = 1;
    tps_read_result res;
    res.best_start = res.best_end = 0;
    res.best_start_idx = res.best_end_idx = 0;
    res.n_win = 0; res.bkp = -1; res.gain = 0.0;
    res.flags = 0; res.reserved = 0;

    if (step1) {
        const int n1 = (int)(L < prm.no_bp ? L : prm.no_bp);
        const uint32_t ks = wide_trc_side(a, l, woff, L, false, n1, has_inv, a.c_start ? a.c_start + r * pat.P : nullptr, 0);
        const uint32_t ke = wide_trc_side(a, l, woff, L, true, n1, has_inv, a.c_end ? a.c_end + r * pat.P : nullptr, 1);
        res.best_start = (int32_t)(ks >> 6); res.best_start_idx = 63 - (int32_t)(ks & 63u);
        res.best_end = (int32_t)(ke >> 6); res.best_end_idx = 63 - (int32_t)(ke & 63u);
        // forward only if strictly larger (allsteps.py:193); strict cutoff and length tests
        tail = res.best_start > res.best_end ? 0 : 1;
        const int best = tail ? res.best_end : res.best_start;
        pass = (L > prm.min_len && best > prm.min_count) ? 1 : 0;
    } else if (a.tails_in) {
        const uint8_t tv = a.tails_in[r];
        tail = tv & 1;
        pass = (tv & 2) ? 0 : 1;                   // bit 1 set = skip this read
    }
    res.tail = tail;
    res.pass = pass;

    int n_win = 0;
    const int64_t out_base = a.win_off ? a.win_off[r] : 0;
    if (pass && (prm.flags & TPS_F_WINDOWS)) {
        const int64_t m_ = L < prm.maxlen ? L : prm.maxlen;
        const int64_t n_s = m_ - prm.trimfirst;
        if (n_s >= prm.window) n_win = (int)((n_s - prm.window) / prm.slide) + 1;
        const int lw1 = prm.window - pat.k > 0 ? prm.window - pat.k : 0;      // start positions of a window of W - 1 characters
        for (int w0 = 0; w0 < n_win; w0 += a.tw) {
            const int nw_tile = (n_win - w0) < a.tw ? (n_win - w0) : a.tw;
            const int m = (nw_tile + NT - 1) / NT;           // consecutive windows per lane
            const int64_t i0 = (int64_t)w0 * prm.slide;
            const int n_stage = (nw_tile - 1) * prm.slide + prm.window - 1;   // <= tp_cap (host) and <= n_s - i0 (the windows exist)
            wide_stage_lookup(a, l, woff, L, tail == 1, prm.trimfirst, i0, n_stage, has_inv);
            const uint64_t sums_g = (uint64_t)(uintptr_t)(a.sums + out_base + w0);
            const uint64_t raw_g = a.raw ? (uint64_t)(uintptr_t)(a.raw + (out_base + w0) * pat.P) : 0ull;
            for (int j = 0; j < m; ++j) {
                TPS_PHASE { wide_step(a, l, j, m, nw_tile, lw1, sums_g, tid); }
                TPS_SYNC();
                if (raw_g) {
                    TPS_PHASE { wide_rows(a, l, j, m, nw_tile, raw_g, tid); }
                    TPS_SYNC();
                }
            }
        }
    }
    res.n_win = n_win;

    if (n_win > 0 && (prm.flags & TPS_F_BINSEG) && binseg_admissible(n_win, prm.jump, prm.min_size)) {
        int bkp;
        double gain;
        bool tie = false;
        TPS_FENCE_WG();                                    // this wave's S_w stores before its own loads
        uint32_t* xs = l.cnt;                              // (the counters are done: XS_DW + MISC_DW + NT dwords fit their region)
        uint32_t* bmisc = xs + ((XS_DW + 1) / 2) * 2;
        uint32_t* bs = bmisc + MISC_DW;
        binseg_wg((const int32_t*)(a.sums + out_base), n_win, prm.jump, prm.min_size, pat.P, bs, bmisc, xs, bkp, gain, tie);
        res.bkp = bkp;
        res.gain = gain;
        res.flags = tie ? TPS_RES_TIE : 0u;
    }
    TPS_PHASE { if (tid == 0) a.results[r] = res; }
}
static_assert(((XS_DW + 1) / 2) * 2 + MISC_DW + NT <= WIDE_CNT_DW, "the change point's scratch must fit the counter region");

// ------------------------------------------------------------------ k-mer followers on a wide table (overview heat map)
// followers_read (tps_device.h) for the tables of tps_set_patterns_wide: up to 32 k-mers of up to 32 letters and any number of
// following letters.  Same semantics, same outputs: in bases [lo, hi) of a read and of its reversed string, the leftmost
// non-overlapping matches of  kmer(.{f})  for patterns 0 .. n_fwd - 1 (strand 0) / n_fwd .. 2 n_fwd - 1 (strand 1), one bit per
// match in picks[read][strand][pattern][pw], and -- where the caller asks and f <= 8 -- the (pattern x followers) histogram.
// One wave per read.  What differs from the narrow kernel:
//   * the look-up is wide_lookup's: one byte per position, group + 1.  A position holds one group; list pattern j reaches its
//     group through pg[] (the two halves of the list may share groups: the 32-letter motif at k = 4 has 58 patterns, 54 groups);
//   * no per-pattern occurrence bitmaps in LDS (32 x 4096 bits would be 16 KB per wave).  The byte map is turned into 32-bit
//     occurrence words a block at a time: lane (pattern j, sub s) compares the 32 bytes of word w0 + s with ITS group -- the lanes
//     of one s read the same 16 bytes (a broadcast) -- and leaves one word in LDS; then lane j < n_fwd walks its NT / n_fwd words of the
//     block leftmost-first with its cursor in a register (a match consumes k + f positions), stores the pick word and, if wanted,
//     adds every pick's followers to the histogram.  The start positions looked up are only those whose f followers lie inside
//     [lo, min(L, hi)), so nothing past them can be picked.
struct FollowWideArgs {
    const uint32_t* seq2;
    const uint16_t* inv;
    const tps_read_desc* desc;
    const uint32_t* img;         // the table image (WIDE_IMG_DW dwords)
    uint32_t* picks;             // [n_reads][2][n_fwd][pw]
    unsigned long long* hist;    // [2][n_fwd][nbins] or nullptr (the host passes it for follow <= 8 only)
    int64_t n_reads;
    WidePat pat;
    int32_t n_fwd, follow, lo, hi, min_len, pw, nbins;
};
constexpr int FOLLOWW_MAX_FWD = 32;
constexpr int FOLLOWW_PM_DW = FOLLOW_MAX_SPAN / 4 + 8;
constexpr int FOLLOWW_VAL_DW = (FOLLOW_SEQ_DW / 2 + 4 + 3) & ~3;       // (a multiple of 4 dwords: the byte map behind it is read and written 16 bytes at a time)
constexpr int FOLLOWW_PM_OFF = FOLLOW_SEQ_DW + FOLLOWW_VAL_DW;
constexpr int FOLLOWW_OCC_OFF = FOLLOWW_PM_OFF + FOLLOWW_PM_DW;
constexpr int FOLLOWW_LDS_DW = (FOLLOWW_OCC_OFF + NT + MISC_DW + 3) & ~3;    // per wave: seq, val, byte map, a block's words, flags
static_assert(FOLLOW_SEQ_DW % 4 == 0 && FOLLOWW_PM_OFF % 4 == 0 && FOLLOWW_PM_DW % 4 == 0 && FOLLOWW_LDS_DW % 4 == 0 && WIDE_IMG_DW % 4 == 0,
              "seq, the byte map and every wave's slice start on 16-byte boundaries (lds_load16 / lds_store16)");
TPS_HD int64_t followers_wide_wg_lds_dwords() { return WIDE_IMG_DW + (int64_t)WPG * FOLLOWW_LDS_DW; }       // (does not depend on n_fwd or the span: sized for 32 and 4096)
// Every refusal of tps_batch_kmer_followers_wide that needs no context, in the library's order (host code; the library and the
// emulation call it): TPS_OK, or the code and *why.  P = the patterns of the table, n = the reads of the batch.
static inline int followers_wide_check(int P, int64_t n, int n_fwd, int follow, int lo, int hi, const void* picks, int64_t picks_words, const void* hist,
                                       int64_t hist_len, Why* why) {
    if (n_fwd < 1 || n_fwd > FOLLOWW_MAX_FWD || 2 * n_fwd > P)
        return refuse(why, TPS_E_ARG, "n_fwd must be 1..%d and the table must hold the complements behind the k-mers", FOLLOWW_MAX_FWD);
    if (follow < 0) return refuse(why, TPS_E_ARG, "follow must not be negative");
    if (lo < 0 || hi <= lo || hi - lo > FOLLOW_MAX_SPAN) return refuse(why, TPS_E_CAPACITY, "the scanned range [lo, hi) must hold 1..%d bases", FOLLOW_MAX_SPAN);
    if (hist && follow > 8) return refuse(why, TPS_E_CAPACITY, "the followers histogram has 4^follow bins: follow must be 0..8 bases with it (pass no hist for more)");
    const int64_t want = n * 2 * n_fwd * ((hi - lo + 31) / 32), bins = hist ? 2ll * n_fwd * ((1 << (2 * follow)) + 1) : 0;
    if (!picks || picks_words != want) return refuse(why, TPS_E_ARG, "picks must hold %lld words", (long long)want);
    if (hist && hist_len != bins) return refuse(why, TPS_E_ARG, "hist must hold %lld counters", (long long)bins);
    return TPS_OK;
}

// bit j = byte j of the 16 equals g1 (g1 >= 1: an empty position never matches)
TPS_DEV uint32_t wide_occ16(const u32x4& v, uint32_t g1) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
    TPS_UNROLL
    for (int j = 0; j < 16; ++j) m |= (((w[j >> 2] >> (8 * (j & 3))) & 255u) == g1 ? 1u : 0u) << j;
    return m;
}

TPS_DEV void followers_wide_read(const FollowWideArgs& a, int64_t r, uint32_t* lds, const uint32_t* img) {
    WideArgs wa{};                                         // what wide_lookup reads of it: the table's description
    wa.pat = a.pat;
    WideLds l{};
    l.seq = lds;
    l.val = (uint16_t*)(lds + FOLLOW_SEQ_DW);
    l.pm = lds + FOLLOWW_PM_OFF;
    uint32_t* occ = lds + FOLLOWW_OCC_OFF;
    l.misc = occ + NT;
    l.tab = img;
    l.pg = (const uint8_t*)(img + WIDE_TAB_DW + WIDE_GM_DW);
    const WidePat& pat = a.pat;
    const int64_t woff = a.desc[r].word_off;
    const int64_t L = a.desc[r].len;
    const bool has_inv = (a.desc[r].flags & TPS_RD_HAS_INVALID) != 0;
    if (L <= a.min_len) return;                    // (the host zeroed the picks)
    const int64_t m = L < a.hi ? L : a.hi;
    const int n = (int)(m - a.lo);
    const int need = pat.k + a.follow;
    if (n < need) return;
    const int npos = n - need + 1;                 // start positions whose followers are inside the range
    const int nch = (npos + 15) >> 4;              // chunks of 16 bytes wide_lookup fills
    const int nwords = (npos + 31) >> 5;           // pick words that can hold a bit (<= pw; the others stay zero)
    const int pw = a.pw;
    const int n_fwd = a.n_fwd;
    const int subs = NT / n_fwd;                   // words of a block
    const uint32_t fmask = a.follow >= 16 ? 0xFFFFFFFFu : ((1u << (2 * a.follow)) - 1u);
    Lane<int> sub, pat_j;                          // the lane's place in a block (one division per read, not per block)
    TPS_LANES { TPS_AT(sub) = tid / n_fwd; TPS_AT(pat_j) = tid - TPS_AT(sub) * n_fwd; }
    for (int strand = 0; strand < 2; ++strand) {
        const Stage st = stage_plan(a.seq2, a.inv, woff, L, strand == 1, a.lo, 0, n);
        TPS_PHASE { if (tid == 0) l.misc[M_INVALID] = 0; }
        TPS_SYNC();
        TPS_PHASE { stage_thread(st, has_inv, l.seq, l.val, st.nq + 1, &l.misc[M_INVALID], tid); }     // (+ a quad of zeros: the last chunk reads three dwords ahead)
        TPS_SYNC();
        const bool any_inv = has_inv && uniform(l.misc[M_INVALID]) != 0;
        TPS_PHASE { wide_lookup(wa, l, st.delta, npos, any_inv, tid); }
        TPS_SYNC();
        Lane<int> cursor(0);
        for (int w0 = 0; w0 < nwords; w0 += subs) {
            TPS_PHASE {
                const int s = TPS_AT(sub), pj = TPS_AT(pat_j), w = w0 + s;
                if (s < subs && w < nwords) {
                    const uint32_t g1 = (uint32_t)l.pg[strand * n_fwd + pj] + 1u;
                    uint32_t mm = wide_occ16(lds_load16(l.pm + 8 * w), g1);
                    if (2 * w + 1 < nch) mm |= wide_occ16(lds_load16(l.pm + 8 * w + 4), g1) << 16;
                    occ[tid] = mm;
                }
            }
            TPS_SYNC();
            TPS_PHASE {
                if (tid < n_fwd) {
                    const uint64_t out_g = (uint64_t)(uintptr_t)(a.picks + ((r * 2 + strand) * n_fwd + tid) * (int64_t)pw);
                    int cur = TPS_AT(cursor);
                    for (int s = 0; s < subs && w0 + s < nwords; ++s) {
                        const int w = w0 + s;
                        uint32_t mm = occ[s * n_fwd + tid], picked = 0;
                        while (mm) {
                            const int bit = ffs0(mm);
                            mm &= mm - 1;
                            const int pos = 32 * w + bit;
                            if (pos < cur) continue;
                            picked |= 1u << bit;
                            cur = pos + need;
                            if (a.hist) {
                                const int q = st.delta + pos + pat.k;
                                uint32_t code = v_at(l.seq, q) & fmask;
                                if (strand) code ^= 0xAAAAAAAAu & fmask;        // complement: A <-> T, C <-> G is code ^ 2
                                const bool bad = any_inv && a.follow > 0 && invalid_at(l.val, q, a.follow);
                                hist_add(&a.hist[((int64_t)strand * n_fwd + tid) * a.nbins + (bad ? (uint32_t)(a.nbins - 1) : code)]);
                            }
                        }
                        g32_store(out_g, (uint32_t)w, picked);
                    }
                    TPS_AT(cursor) = cur;
                }
            }
            TPS_SYNC();
        }
    }
}
static_assert(NT / FOLLOWW_MAX_FWD >= 1, "a block holds at least one word per pattern");

}  // namespace tps
