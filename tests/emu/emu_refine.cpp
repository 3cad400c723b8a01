// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the boundary refinement kernel (refine_read, topsicle_amd/csrc/tps_refine.h).
//
// Like emu_adapter.cpp: the header compiled with -DTPS_EMU, the batch packed by the library's own packer, the argument checks of
// tps_batch_boundary_refine (the library's own: boundary_refine_check) with its return codes, the hit table built by the function
// the library calls.  Never linked into the product.  emu_refine_main.cpp includes this file and adds a main() for the stand-alone
// sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_refine.h"
#include "emu_batch.h"

static std::string g_err;
extern "C" const char* emu_refine_last_error() { return g_err.c_str(); }

// tps_batch_upload + tps_batch_boundary_refine.  base_shift moves the batch inside its buffer by whole quads; words the layout does
// not own are garbage.
extern "C" int emu_boundary_refine(const uint8_t* bases, const int64_t* offsets, int64_t n, uint64_t unit, int m, const uint8_t* tails, const int32_t* begin,
                                   const int32_t* end, const int32_t* at, int64_t n_reads, int hit, int miss, int sep, int base_shift, tps_refine* out,
                                   int64_t out_len) {
    tps::Why why;
    if (const int rc = tps::boundary_refine_check(n, offsets, unit, m, tails, begin, end, at, n_reads, hit, miss, sep, out, out_len, &why)) { g_err = why.msg; return rc; }
    if (n == 0) return TPS_OK;
    const emu::Batch batch(bases, offsets, n, base_shift);
    const int w = m < tps::TRACT_MAX_WORD ? m : tps::TRACT_MAX_WORD;
    // the table and the rows of exactly their sizes: a sanitizer build sees an access past them (the kernel writes every row whole)
    std::vector<uint32_t> table((size_t)tps::tract_table_dw(w));
    tps::tract_hit_table(unit, m, table.data());
    std::vector<tps_refine> rows((size_t)n);
    memset(rows.data(), 0xEE, rows.size() * sizeof(tps_refine));
    tps::RefineArgs a{};
    batch.set(a);
    a.table = table.data();
    a.tails = tails; a.begin = begin; a.end = end; a.at = at;
    a.out = rows.data(); a.n_reads = n;
    a.w = w; a.hit = hit; a.miss = miss; a.sep = sep;
    a.bal_dw = tps::refine_ballot_dw(n, offsets, begin, end, w);
    emu::WaveLds lds(tps::refine_lds_dw(a.bal_dw));          // exactly the slice the library gives a wave
    for (int64_t r = 0; r < n; ++r) tps::refine_read(a, r, lds.poisoned(), table.data());
    memcpy(out, rows.data(), rows.size() * sizeof(tps_refine));
    return TPS_OK;
}

extern "C" int emu_refine_piece() { return tps::REFINE_PIECE; }
extern "C" int emu_refine_wpg() { return tps::REFINE_WPG; }
