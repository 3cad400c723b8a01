// tps_wide_plan.h -- host side of the wide-table scan (tps_wide.h), shared by the library (topsicle_hip.hip) and the test
// emulation (tests/emu/emu_wide.cpp): pattern list -> hash table image, and the LDS plan of one scan.  Plain C++, no HIP calls.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "tps_wide.h"

namespace tps {

// Pattern list (P strings of k letters, reference order) -> WideArgs::img and WidePat.  Returns "" or an error message.
inline std::string build_wide_table(const char* pats, int P, int k, std::vector<uint32_t>& img, WidePat& wp) {
    if (k < 1 || k > TPS_WIDE_MAX_K) return "k=" + std::to_string(k) + " not supported (1.." + std::to_string(TPS_WIDE_MAX_K) + ")";
    if (P < 1 || P > TPS_WIDE_MAX_PATTERNS) return std::to_string(P) + " patterns not supported (1.." + std::to_string(TPS_WIDE_MAX_PATTERNS) + ")";
    std::vector<uint64_t> codes((size_t)P);
    std::vector<uint8_t> so((size_t)P, 0);
    for (int p = 0; p < P; ++p) {
        uint64_t code = 0;
        char up[TPS_WIDE_MAX_K];
        for (int i = 0; i < k; ++i) {
            char ch = pats[(size_t)p * k + i];
            if (ch >= 'a' && ch <= 'z') ch = (char)(ch - 32);
            up[i] = ch;
            uint64_t v;
            switch (ch) {          // the 2-bit code of the packed batch: (ASCII >> 1) & 3
                case 'A': v = 0; break;
                case 'C': v = 1; break;
                case 'T': v = 2; break;
                case 'G': v = 3; break;
                default: return "pattern " + std::to_string(p) + " has a non-ACGT letter";
            }
            code |= v << (2 * i);
        }
        codes[(size_t)p] = code;
        for (int d = 1; d < k && !so[(size_t)p]; ++d) {        // a proper period: the k-mer can overlap itself
            bool periodic = true;
            for (int i = 0; i + d < k; ++i) periodic = periodic && (up[i] == up[i + d]);
            if (periodic) so[(size_t)p] = 1;
        }
    }
    // groups = distinct codes, the self-overlapping ones first, otherwise in list order
    std::vector<uint64_t> gcode;
    std::vector<int> pg((size_t)P, -1);
    for (int pass = 0; pass < 2; ++pass)
        for (int p = 0; p < P; ++p) {
            if ((so[(size_t)p] != 0) != (pass == 0) || pg[(size_t)p] >= 0) continue;
            int g = -1;
            for (size_t i = 0; i < gcode.size(); ++i) if (gcode[i] == codes[(size_t)p]) g = (int)i;
            if (g < 0) { g = (int)gcode.size(); gcode.push_back(codes[(size_t)p]); }
            pg[(size_t)p] = g;
        }
    wp = WidePat{};
    wp.P = P;
    wp.k = k;
    wp.n_groups = (int)gcode.size();
    for (int p = 0; p < P; ++p) if (so[(size_t)p] && pg[(size_t)p] + 1 > wp.n_so) wp.n_so = pg[(size_t)p] + 1;
    const uint64_t mask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1ull);
    wp.mask_lo = (uint32_t)mask;
    wp.mask_hi = (uint32_t)(mask >> 32);
    // a rotation and an odd multiplier under which no two codes share a slot
    auto slot_of = [](uint64_t code, uint32_t rot, uint32_t mul) {
        const uint32_t lo = (uint32_t)code, hi = (uint32_t)(code >> 32);
        const uint32_t f = lo + (rot ? ((hi >> rot) | (hi << (32 - rot))) : hi);
        return (f * mul) >> 24;
    };
    bool found = false;
    for (uint32_t rot = 0; rot < 32 && !found; ++rot)
        for (uint32_t cand = 0x9E3779B1u, tries = 0; tries < 20000 && !found; ++tries, cand += 0xC657CB56u) {
            const uint32_t mul = cand | 1u;
            bool used[WIDE_SLOTS] = {false};
            bool ok = true;
            for (size_t g = 0; g < gcode.size() && ok; ++g) {
                const uint32_t s = slot_of(gcode[g], rot, mul);
                if (used[s]) ok = false;
                used[s] = true;
            }
            if (ok) { wp.rot = rot; wp.mul = mul; found = true; }
        }
    if (!found) return "no collision-free hash for this pattern table";
    img.assign((size_t)WIDE_IMG_DW, 0u);
    for (size_t g = 0; g < gcode.size(); ++g) {
        const uint32_t s = slot_of(gcode[g], wp.rot, wp.mul);
        img[4 * s] = (uint32_t)gcode[g];
        img[4 * s + 1] = (uint32_t)(gcode[g] >> 32);
        img[4 * s + 2] = (uint32_t)g + 1u;               // 0 = unused slot: no code is reserved as a marker
    }
    uint8_t* pgb = (uint8_t*)&img[WIDE_TAB_DW + WIDE_GM_DW];
    for (int p = 0; p < P; ++p) {
        img[(size_t)WIDE_TAB_DW + (size_t)pg[(size_t)p]] += 1u;
        pgb[p] = (uint8_t)pg[(size_t)p];
    }
    return "";
}

// LDS plan of one scan: tp_cap, tw, seq_dw, wpg.  budget_dw = LDS dwords one workgroup may use.
inline std::string plan_wide(WideArgs& a, const tps_params& prm, int64_t budget_dw) {
    int64_t tp = WIDE_TP_MIN;
    if (prm.flags & TPS_F_WINDOWS) {
        // a lane's counters are bytes, like the raw rows: bounded by what a window can hold of one k-mer
        if ((prm.window - 1) / a.pat.k > 255)
            return "a window of " + std::to_string(prm.window) + " can hold more than 255 occurrences of a " + std::to_string(a.pat.k) + "-mer";
        if (prm.window - 1 > tp) tp = prm.window - 1;
    }
    if ((prm.flags & TPS_F_STEP1) && prm.no_bp > tp) tp = prm.no_bp;
    tp = (tp + 63) & ~63ll;
    if (tp > WIDE_TP_MAX) return "window / step-1 head of more than " + std::to_string(WIDE_TP_MAX) + " bases";
    a.tp_cap = (int32_t)tp;
    int64_t tw = (tp - (prm.window - 1)) / prm.slide + 1;
    if (tw < 1) tw = 1;
    if (tw >= NT) tw &= ~(int64_t)(NT - 1);                // every lane the same number of windows
    a.tw = (int32_t)tw;
    a.seq_dw = (int32_t)(4 * ((63 + tp + 63) / 64 + 2));
    a.wpg = WPG;
    if (wide_wg_lds_dwords(a) > budget_dw) return "the wide kernel's LDS plan does not fit";
    return "";
}

}  // namespace tps
