// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the base-modification kernel (mod_read, topsicle_amd/csrc/tps_methyl.h).
//
// Like emu_refine.cpp: the header compiled with -DTPS_EMU, the batch packed by the library's own packer, the argument checks of
// tps_batch_mod_profile (the library's own: mod_profile_check) with its return codes.  Never linked into the product.
// emu_methyl_main.cpp includes this file and adds a main() for the stand-alone sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_methyl.h"
#include "emu_batch.h"

static std::string g_err;
extern "C" const char* emu_methyl_last_error() { return g_err.c_str(); }

// tps_batch_upload + tps_batch_mod_profile.  base_shift moves the batch inside its buffer by whole quads; words the layout does not
// own are garbage.
extern "C" int emu_mod_profile(const uint8_t* bases, const int64_t* offsets, int64_t n, const uint8_t* tails, const int32_t* begin, const int32_t* end,
                               const int32_t* origin, int64_t n_reads, const int64_t* mod_off, const uint32_t* delta, const uint8_t* prob, int64_t n_mods, int w,
                               int nb0, int nb1, int hi, int lo, int base_shift, tps_mod_row* rows, int64_t rows_len, tps_mod_bin* bins, int64_t bins_len) {
    tps::Why why;
    if (const int rc = tps::mod_profile_check(n, offsets, tails, begin, end, origin, n_reads, mod_off, delta, prob, n_mods, w, nb0, nb1, hi, lo, rows, rows_len, bins,
                                              bins_len, &why)) {
        g_err = why.msg;
        return rc;
    }
    if (n == 0) return TPS_OK;
    const emu::Batch batch(bases, offsets, n, base_shift);
    // the entries, the rows and the bins of exactly their sizes: a sanitizer build sees an access past them (the kernel writes every
    // row and every record whole)
    std::vector<uint32_t> d(delta, delta + n_mods);
    std::vector<uint8_t> p(prob, prob + n_mods);
    std::vector<tps_mod_row> r_out((size_t)n);
    std::vector<tps_mod_bin> b_out((size_t)(n * (nb0 + nb1)));
    memset(r_out.data(), 0xEE, r_out.size() * sizeof(tps_mod_row));
    memset(b_out.data(), 0xEE, b_out.size() * sizeof(tps_mod_bin));
    tps::ModArgs a{};
    batch.set(a);
    a.tails = tails; a.begin = begin; a.end = end; a.origin = origin;
    a.mod_off = mod_off; a.delta = d.data(); a.prob = p.data();
    a.rows = r_out.data(); a.bins = b_out.data(); a.n_reads = n;
    a.w = w; a.nb0 = nb0; a.nb1 = nb1; a.hi = hi; a.lo = lo;
    emu::WaveLds lds(tps::MOD_LDS_DW);                       // exactly the slice the library gives a wave
    for (int64_t r = 0; r < n; ++r) tps::mod_read(a, r, lds.poisoned());
    memcpy(rows, r_out.data(), r_out.size() * sizeof(tps_mod_row));
    memcpy(bins, b_out.data(), b_out.size() * sizeof(tps_mod_bin));
    return TPS_OK;
}

extern "C" int emu_methyl_wpg() { return tps::MOD_WPG; }
extern "C" int emu_methyl_max_region() { return tps::MOD_MAX_REGION; }
