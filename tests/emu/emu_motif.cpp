// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the motif census kernel (motif_read, topsicle_amd/csrc/tps_motif.h).
//
// Like emu_follow_wide.cpp: the header compiled with -DTPS_EMU, the batch packed by the library's own packer, the argument checks of
// tps_batch_motif_census the library's own (motif_census_check).  Never linked into the product.  emu_motif_main.cpp includes this file and
// adds a main() for the stand-alone sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_motif.h"
#include "emu_batch.h"

static std::string g_err;
extern "C" const char* emu_motif_last_error() { return g_err.c_str(); }

// tps_batch_upload + tps_batch_motif_census: hits[n][2], counts[n][2][u_max - u_min + 1] or NULL.  base_shift moves the batch inside
// its buffer by whole quads; words the layout does not own are garbage.
extern "C" int emu_motif_census(const uint8_t* bases, const int64_t* offsets, int64_t n, int u_min, int u_max, int lo, int hi, int min_len,
                                int base_shift, tps_motif_hit* hits, int64_t n_hits, int32_t* counts, int64_t counts_len) {
    tps::Why why;
    if (const int rc = tps::motif_census_check(n, u_min, u_max, lo, hi, hits, n_hits, counts, counts_len, &why)) { g_err = why.msg; return rc; }
    if (n == 0) return TPS_OK;
    const emu::Batch batch(bases, offsets, n, base_shift);
    memset(hits, 0, (size_t)n_hits * sizeof(tps_motif_hit));                  // (the library's hipMemsetAsync)
    if (counts) memset(counts, 0, (size_t)counts_len * 4);
    tps::MotifArgs a{};
    batch.set(a);
    a.hits = hits; a.counts = counts; a.n_reads = n;
    a.u_min = u_min; a.u_max = u_max; a.lo = lo; a.hi = hi; a.min_len = min_len;
    emu::WaveLds lds(tps::MOTIF_LDS_DW);
    for (int64_t r = 0; r < n; ++r) tps::motif_read(a, r, lds.poisoned());
    return TPS_OK;
}
