// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the placement kernel (window_place_row, topsicle_amd/csrc/tps_place.h).
//
// Like emu_anchor.cpp: the header compiled with -DTPS_EMU, the argument checks of tps_window_place (the library's own:
// window_place_check) with its return codes, the index built by the function the library calls (place_index_build).  Never linked
// into the product.  emu_place_main.cpp includes this file and adds a main() for the stand-alone sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_place.h"
#include "emu_batch.h"

static std::string g_place_err;
static int g_place_bits = 0;
extern "C" const char* emu_place_last_error() { return g_place_err.c_str(); }
// the bits of the directory the last call built (the tests check that their k-mers lie where they say)
extern "C" int emu_place_dir_bits() { return g_place_bits; }

// tps_window_place; outs = the seven outputs behind one another, int32[7][n]
extern "C" int emu_window_place(const uint32_t* codes, int64_t codes_len, const uint32_t* keep, int64_t keep_len, const int32_t* length, int64_t n,
                                const uint32_t* ref_codes, int64_t ref_codes_len, const uint32_t* ref_keep, int64_t ref_keep_len, const int32_t* ref_length,
                                int n_ref, int span, int k, int max_occ, int32_t* outs, int64_t out_len) {
    tps::Why why;
    if (const int rc = tps::window_place_check(codes, codes_len, keep, keep_len, length, n, ref_codes, ref_codes_len, ref_keep, ref_keep_len, ref_length, n_ref,
                                               span, k, max_occ, outs != nullptr, out_len, &why)) {
        g_place_err = why.msg;
        return rc;
    }
    if (n == 0) return TPS_OK;
    const int cdw = (span + 15) / 16, kdw = (span + 31) / 32;
    // exactly the rows and the index, as the device buffers are long: a sanitizer build sees a load past them
    std::vector<uint32_t> rc_(ref_codes, ref_codes + (int64_t)n_ref * cdw), rk_(ref_keep, ref_keep + (int64_t)n_ref * kdw);
    std::vector<int32_t> rl_(ref_length, ref_length + n_ref);
    tps::PlaceIndex ix;
    tps::place_index_build(rc_.data(), rk_.data(), rl_.data(), n_ref, cdw, kdw, k, max_occ, ix);
    g_place_bits = ix.bits;
    ix.dir.shrink_to_fit(); ix.keys.shrink_to_fit(); ix.ent.shrink_to_fit();
    std::vector<uint32_t> co(codes, codes + n * cdw), kp(keep, keep + n * kdw);
    std::vector<int32_t> ln(length, length + n);
    std::vector<int32_t> out((size_t)(tps::PLACE_OUTS * n), (int32_t)0xEEEEEEEE);       // (the kernel writes every entry)
    tps::PlaceArgs a{};
    a.codes = co.data(); a.keep = kp.data(); a.length = ln.data();
    a.dir = ix.dir.data(); a.keys = ix.keys.data(); a.ent = ix.ent.data();
    a.out = out.data();
    a.n = n;
    a.R = n_ref; a.k = k; a.cdw = cdw; a.kdw = kdw; a.shift = 32 - ix.bits;
    emu::WaveLds lds(tps::PLACE_LDS_DW);
    for (int64_t i = 0; i < n; ++i) tps::window_place_row(a, i, lds.poisoned());
    memcpy(outs, out.data(), out.size() * 4);
    return TPS_OK;
}
