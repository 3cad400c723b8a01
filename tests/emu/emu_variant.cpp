// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the variant census kernel (variant_read, topsicle_amd/csrc/tps_variant.h).
//
// Like emu_motif.cpp: the header compiled with -DTPS_EMU, the batch packed by the library's own packer, the argument checks of
// tps_batch_variant_census restated with its return codes, its partial profiles added up as the library adds them.  Never linked
// into the product.  emu_variant_main.cpp includes this file and adds a main() for the stand-alone sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_variant.h"
#include "../../topsicle_amd/csrc/tps_pack.h"

static std::string g_err;
extern "C" const char* emu_variant_last_error() { return g_err.c_str(); }

// tps_batch_upload + tps_batch_variant_census: counts[n][2 + 4m], profile[n_bins][2 + 4m] or NULL.  base_shift moves the batch
// inside its buffer by whole quads; words the layout does not own are garbage.
extern "C" int emu_variant_census(const uint8_t* bases, const int64_t* offsets, int64_t n, uint64_t unit, int m, const uint8_t* tails,
                                  const int32_t* begin, const int32_t* end, int64_t n_reads, int bin, int n_bins, int base_shift,
                                  uint32_t* counts, int64_t counts_len, int64_t* profile, int64_t profile_len) {
    if (m < 2 || m > tps::VARIANT_MAX_UNIT) { g_err = "the unit must have 2..32 letters"; return TPS_E_ARG; }
    if (m < 32 && (unit >> (2 * m)) != 0) { g_err = "the unit has codes behind its letters"; return TPS_E_ARG; }
    for (int d = 1; d < m; ++d) {
        if (m % d) continue;
        const uint64_t rot = (unit >> (2 * d)) | (unit << (2 * (m - d)));
        if (((rot ^ unit) & (~0ull >> (64 - 2 * m))) == 0) { g_err = "the unit is a power of a shorter word"; return TPS_E_ARG; }
    }
    if (bin < tps::VARIANT_MIN_BIN || bin > tps::VARIANT_MAX_BIN) { g_err = "bin must be 64..4064 positions"; return TPS_E_CAPACITY; }
    if (n_bins < 1 || n_bins > tps::VARIANT_MAX_BINS) { g_err = "n_bins must be 1..64"; return TPS_E_CAPACITY; }
    const int cols = 2 + 4 * m;
    if (n_reads != n) { g_err = "tails, begin and end must hold n reads"; return TPS_E_ARG; }
    if (n > 0 && (!tails || !begin || !end)) { g_err = "null tails / begin / end"; return TPS_E_ARG; }
    if ((!counts && n > 0) || counts_len != n * cols) { g_err = "counts must hold n (2 + 4m) counters"; return TPS_E_ARG; }
    if (profile && profile_len != (int64_t)n_bins * cols) { g_err = "profile must hold n_bins (2 + 4m) counters"; return TPS_E_ARG; }
    for (int64_t i = 0; i < n; ++i) {
        if (tails[i] > 1) { g_err = "tail must be 0 or 1"; return TPS_E_ARG; }
        if (begin[i] < 0 || end[i] < 0 || begin[i] > end[i]) { g_err = "need 0 <= begin <= end"; return TPS_E_ARG; }
    }
    if (profile) memset(profile, 0, (size_t)profile_len * 8);
    if (n == 0) return TPS_OK;
    std::vector<tps_read_desc> desc((size_t)n);
    const int64_t n_words = tps::pack_layout(offsets, n, desc.data());
    const int64_t lead = 4 * (int64_t)(base_shift & 3);
    std::vector<uint32_t> seq2buf((size_t)(n_words + lead + 8), 0xDEADBEEFu);
    std::vector<uint16_t> invbuf((size_t)(n_words + lead + 8), (uint16_t)0xFFFFu);
    for (int64_t i = 0; i < n; ++i) desc[(size_t)i].word_off += lead;
    tps::pack_range(bases, offsets, 0, n, desc.data(), seq2buf.data(), invbuf.data());
    memset(counts, 0, (size_t)counts_len * 4);                                // (the library's hipMemsetAsync)
    const size_t part_len = (size_t)n_bins * cols;
    std::vector<unsigned long long> parts(profile ? tps::VARIANT_PARTS * part_len : 0, 0ull);
    tps::VariantArgs a{};
    a.seq2 = seq2buf.data(); a.inv = invbuf.data(); a.desc = desc.data();
    a.tails = tails; a.begin = begin; a.end = end;
    a.counts = counts; a.prof = profile ? parts.data() : nullptr; a.n_reads = n;
    a.unit = unit; a.m = m; a.bin = bin; a.n_bins = n_bins;
    // exactly one wave's slice, 16-byte aligned like LDS: a sanitizer build sees every access past it
    uint32_t* lds = nullptr;
    if (posix_memalign((void**)&lds, 16, (size_t)tps::VARIANT_LDS_DW * 4)) { g_err = "out of memory"; return TPS_E_ARG; }
    for (int64_t r = 0; r < n; ++r) {
        for (int i = 0; i < tps::VARIANT_LDS_DW; ++i) lds[i] = 0xDEADBEEFu;     // LDS content is undefined at workgroup start
        tps::variant_read(a, r, lds, (int)((r / tps::WPG) % tps::VARIANT_PARTS));
    }
    free(lds);
    if (profile)
        for (int p = 0; p < tps::VARIANT_PARTS; ++p)
            for (size_t i = 0; i < part_len; ++i) profile[i] += (int64_t)parts[p * part_len + i];
    return TPS_OK;
}
