// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the tract map kernel (tract_read, topsicle_amd/csrc/tps_tract.h).
//
// Like emu_variant.cpp: the header compiled with -DTPS_EMU, the batch packed by the library's own packer, the argument checks of
// tps_batch_tract_map (tract_map_check, the library's own) with its return codes, the hit table built by the function the library calls.
// Never linked into the product.  emu_tract_main.cpp includes this file and adds a main() for the stand-alone sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_tract.h"
#include "emu_batch.h"

static std::string g_err;
extern "C" const char* emu_tract_last_error() { return g_err.c_str(); }

// positions of a staged piece (the seam cases are built from it)
extern "C" int emu_tract_piece(int block) { return tps::tract_piece(block); }

// the hit table of a unit as the library builds it: tab[4^min(m, 8) / 16]
extern "C" int emu_tract_table(uint64_t unit, int m, uint32_t* tab) {
    if (m < tps::TRACT_MIN_UNIT || m > tps::TRACT_MAX_UNIT) return TPS_E_ARG;
    tps::tract_hit_table(unit, m, tab);
    return TPS_OK;
}

// tps_batch_upload + tps_batch_tract_map.  base_shift moves the batch inside its buffer by whole quads; words the layout does not
// own are garbage.
extern "C" int emu_tract_map(const uint8_t* bases, const int64_t* offsets, int64_t n, uint64_t unit, int m, int block, int min_hits, int gap,
                             int min_blocks, int max_tracts, int base_shift, tps_tract* tracts, int64_t tracts_len, int32_t* found,
                             int64_t found_len, uint32_t* totals, int64_t totals_len) {
    tps::Why why;
    if (const int rc = tps::tract_map_check(n, unit, m, block, min_hits, gap, min_blocks, max_tracts, tracts, tracts_len, found, found_len, totals, totals_len, &why)) {
        g_err = why.msg;
        return rc;
    }
    if (n == 0) return TPS_OK;
    const emu::Batch batch(bases, offsets, n, base_shift);
    memset(tracts, 0, (size_t)tracts_len * sizeof(tps_tract));                // (the library's hipMemsetAsync)
    memset(found, 0xEE, (size_t)found_len * 4);                               // (the kernel writes every entry of these two)
    memset(totals, 0xEE, (size_t)totals_len * 4);
    const int w = m < tps::TRACT_MAX_WORD ? m : tps::TRACT_MAX_WORD;
    std::vector<uint32_t> table((size_t)tps::tract_table_dw(w));              // exactly the table: a sanitizer build sees a look-up past it
    tps::tract_hit_table(unit, m, table.data());
    tps::TractArgs a{};
    batch.set(a);
    a.table = table.data();
    a.tracts = tracts; a.found = found; a.totals = totals; a.n_reads = n;
    a.w = w; a.block = block; a.min_hits = min_hits; a.gap = gap; a.min_blocks = min_blocks; a.max_tracts = max_tracts;
    emu::WaveLds lds(tps::TRACT_LDS_DW);
    for (int64_t r = 0; r < n; ++r) tps::tract_read(a, r, lds.poisoned(), a.table);
    return TPS_OK;
}
