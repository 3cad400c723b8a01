// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the variant census kernel (variant_read, topsicle_amd/csrc/tps_variant.h).
//
// Like emu_motif.cpp: the header compiled with -DTPS_EMU, the batch packed by the library's own packer, the argument checks of
// tps_batch_variant_census the library's own (variant_census_check), its partial profiles added up as the library adds them.  Never linked
// into the product.  emu_variant_main.cpp includes this file and adds a main() for the stand-alone sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_variant.h"
#include "emu_batch.h"

static std::string g_err;
extern "C" const char* emu_variant_last_error() { return g_err.c_str(); }

// tps_batch_upload + tps_batch_variant_census: counts[n][2 + 4m], profile[n_bins][2 + 4m] or NULL.  base_shift moves the batch
// inside its buffer by whole quads; words the layout does not own are garbage.
extern "C" int emu_variant_census(const uint8_t* bases, const int64_t* offsets, int64_t n, uint64_t unit, int m, const uint8_t* tails,
                                  const int32_t* begin, const int32_t* end, int64_t n_reads, int bin, int n_bins, int base_shift,
                                  uint32_t* counts, int64_t counts_len, int64_t* profile, int64_t profile_len) {
    tps::Why why;
    if (const int rc = tps::variant_census_check(n, unit, m, tails, begin, end, n_reads, bin, n_bins, counts, counts_len, profile, profile_len, &why)) {
        g_err = why.msg;
        return rc;
    }
    const int cols = 2 + 4 * m;
    if (profile) memset(profile, 0, (size_t)profile_len * 8);
    if (n == 0) return TPS_OK;
    const emu::Batch batch(bases, offsets, n, base_shift);
    memset(counts, 0, (size_t)counts_len * 4);                                // (the library's hipMemsetAsync)
    const size_t part_len = (size_t)n_bins * cols;
    std::vector<unsigned long long> parts(profile ? tps::VARIANT_PARTS * part_len : 0, 0ull);
    tps::VariantArgs a{};
    batch.set(a);
    a.tails = tails; a.begin = begin; a.end = end;
    a.counts = counts; a.prof = profile ? parts.data() : nullptr; a.n_reads = n;
    a.unit = unit; a.m = m; a.bin = bin; a.n_bins = n_bins;
    emu::WaveLds lds(tps::VARIANT_LDS_DW);
    for (int64_t r = 0; r < n; ++r) tps::variant_read(a, r, lds.poisoned(), (int)((r / tps::WPG) % tps::VARIANT_PARTS));
    if (profile)
        for (int p = 0; p < tps::VARIANT_PARTS; ++p)
            for (size_t i = 0; i < part_len; ++i) profile[i] += (int64_t)parts[p * part_len + i];
    return TPS_OK;
}
