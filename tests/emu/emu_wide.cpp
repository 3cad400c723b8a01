// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the wide-table scan kernel (topsicle_amd/csrc/tps_wide.h).
//
// Like emu_scan.cpp for tps_device.h: the header compiled with -DTPS_EMU, TPS_PHASE looping over the 64 lane ids, the table and
// the LDS plan built by the very functions the library calls (tps_wide_plan.h).  Never linked into the product.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_wide.h"
#include "../../topsicle_amd/csrc/tps_wide_plan.h"
#include "emu_batch.h"
#include "../../topsicle_amd/csrc/tps_plan.h"

static std::string g_err;
extern "C" const char* emu_wide_last_error() { return g_err.c_str(); }

// the table alone: rc, and out8 = {n_groups, n_so, rot, mul, used slots, mask_lo, mask_hi, 0}
extern "C" int emu_wide_table(const char* pats, int P, int k, uint32_t* out8) {
    std::vector<uint32_t> img;
    tps::WidePat wp;
    std::string err = tps::build_wide_table(pats, P, k, img, wp);
    if (!err.empty()) { g_err = err; return TPS_E_PATTERN; }
    uint32_t used = 0;
    for (int s = 0; s < tps::WIDE_SLOTS; ++s) used += img[4 * (size_t)s + 2] != 0;
    out8[0] = (uint32_t)wp.n_groups; out8[1] = (uint32_t)wp.n_so; out8[2] = wp.rot; out8[3] = wp.mul; out8[4] = used;
    out8[5] = wp.mask_lo; out8[6] = wp.mask_hi; out8[7] = 0;
    return TPS_OK;
}

// the LDS plan alone, as do_scan decides it for a device whose workgroups may use budget_bytes of LDS: rc (TPS_E_CAPACITY: the plan
// refuses, emu_wide_last_error says why), and out8 = {tp_cap, tw, seq_dw, wpg, workgroup LDS bytes, n_so, 0, 0}
extern "C" int emu_wide_plan(const char* pats, int P, int k, const tps_params* prm, int64_t budget_bytes, int64_t* out8) {
    std::vector<uint32_t> img;
    tps::WideArgs a{};
    std::string err = tps::build_wide_table(pats, P, k, img, a.pat);
    if (!err.empty()) { g_err = err; return TPS_E_PATTERN; }
    if (prm->window < 1 || prm->slide < 1 || prm->trimfirst < 0 || prm->maxlen < 0 || prm->no_bp < 0) { g_err = "bad window/slide/trimfirst/maxlen/no_bp"; return TPS_E_ARG; }
    err = tps::plan_wide(a, *prm, budget_bytes / 4);
    if (!err.empty()) { g_err = err; return TPS_E_CAPACITY; }
    out8[0] = a.tp_cap; out8[1] = a.tw; out8[2] = a.seq_dw; out8[3] = a.wpg; out8[4] = tps::wide_wg_lds_dwords(a) * 4;
    out8[5] = a.pat.n_so; out8[6] = out8[7] = 0;
    return TPS_OK;
}

// One scan over a batch, like tps_set_patterns_wide + tps_batch_upload + tps_batch_scan + downloads.  base_shift moves the
// batch inside its buffer by whole quads; words the layout does not own are garbage.
extern "C" int emu_wide_scan(const char* pats, int P, int k, const uint8_t* bases, const int64_t* offsets, int64_t n,
                             const uint8_t* tails, const tps_params* prm, int base_shift, tps_read_result* results,
                             int32_t* c_start, int32_t* c_end, int64_t* win_off_out, int32_t* sums, uint8_t* raw) {
    std::vector<uint32_t> img;
    tps::WideArgs a{};
    std::string err = tps::build_wide_table(pats, P, k, img, a.pat);
    if (!err.empty()) { g_err = err; return TPS_E_PATTERN; }
    if (prm->window < 1 || prm->slide < 1 || prm->trimfirst < 0 || prm->maxlen < 0 || prm->no_bp < 0) { g_err = "bad window/slide/trimfirst/maxlen/no_bp"; return TPS_E_ARG; }
    err = tps::plan_wide(a, *prm, 160 * 1024 / 4);
    if (!err.empty()) { g_err = err; return TPS_E_CAPACITY; }
    // window layout and dispatch order as the library plans them (the wide kernel has no 16-bit sums: win_off16 is not used)
    tps::BatchLayout lay;
    tps::plan_batch_layout(offsets, n, *prm, lay);
    const std::vector<int64_t>& win_off = lay.win_off;
    if (win_off_out) memcpy(win_off_out, win_off.data(), (size_t)(n + 1) * 8);

    const emu::Batch batch(bases, offsets, n, base_shift);
    batch.set(a);
    a.tails_in = ((prm->flags & TPS_F_TAILS_IN) && !(prm->flags & TPS_F_STEP1)) ? tails : nullptr;
    a.results = results;
    a.c_start = (prm->flags & TPS_F_STEP1) ? c_start : nullptr;
    a.c_end = (prm->flags & TPS_F_STEP1) ? c_end : nullptr;
    a.win_off = win_off.data();
    a.sums = sums;
    a.raw = (prm->flags & TPS_F_STORE_RAW) ? raw : nullptr;
    a.n_reads = n;
    a.prm = *prm;
    // the workgroup's copy of the table image, 16-byte aligned like LDS
    std::vector<uint32_t> imgbuf((size_t)tps::WIDE_IMG_DW + 4);
    uint32_t* img_al = (uint32_t*)(((uintptr_t)imgbuf.data() + 15) & ~(uintptr_t)15);
    memcpy(img_al, img.data(), (size_t)tps::WIDE_IMG_DW * 4);
    a.img = img_al;
    // exactly the planned wave slice: the sanitizer build sees every access past it
    emu::WaveLds lds((int)tps::wide_lds_dwords(a));
    for (int64_t slot = 0; slot < n; ++slot) {
        const int64_t r = lay.order.empty() ? slot : lay.order[(size_t)slot];       // (results do not depend on the order)
        tps::wide_read(a, r, lds.poisoned(), img_al);
    }
    return TPS_OK;
}
