// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the banded alignment kernel (window_align_row,
// topsicle_amd/csrc/tps_align.h).
//
// Like emu_anchor.cpp: the header compiled with -DTPS_EMU, the argument checks of tps_window_align (the library's own:
// window_align_check) with their return codes, the wave's LDS slice sized by the function the library calls.  Never linked into the
// product.  emu_align_main.cpp includes this file and adds a main() for the stand-alone sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_align.h"
#include "emu_batch.h"

static std::string g_err;
extern "C" const char* emu_align_last_error() { return g_err.c_str(); }

// tps_window_align
extern "C" int emu_window_align(const uint32_t* codes, int64_t codes_len, const int32_t* length, int64_t n, const uint32_t* ref_codes, int64_t ref_codes_len,
                                const int32_t* ref_length, int32_t n_ref, const int32_t* ref, const int32_t* centre, int32_t span, int32_t* stat,
                                int64_t stat_len, uint16_t* cols, int64_t cols_len, const int32_t* pile_row, int32_t* pile, int32_t n_pile, int64_t pile_len) {
    tps::Why why;
    if (const int rc = tps::window_align_check(codes, codes_len, length, n, ref_codes, ref_codes_len, ref_length, n_ref, ref, centre, span, stat, stat_len, cols,
                                               cols_len, pile_row, pile, n_pile, pile_len, &why)) {
        g_err = why.msg;
        return rc;
    }
    if (n == 0) {
        if (pile) memset(pile, 0, (size_t)pile_len * 4);
        return TPS_OK;
    }
    const int cdw = (span + 15) / 16;
    // exactly the rows, as the device buffers are long: a sanitizer build sees an access past them
    std::vector<uint32_t> co(codes, codes + n * cdw), rco(ref_codes, ref_codes + (int64_t)n_ref * cdw);
    std::vector<int32_t> len(length, length + n), rlen(ref_length, ref_length + n_ref), rf(ref, ref + n), ce(centre, centre + n), pr;
    if (pile_row) pr.assign(pile_row, pile_row + n);
    std::vector<int32_t> st((size_t)stat_len, (int32_t)0xEEEEEEEE);             // (the kernel writes every entry)
    std::vector<uint16_t> cl((size_t)cols_len, (uint16_t)0xEEEE);
    std::vector<int32_t> pl((size_t)(pile ? pile_len : 0), 0);                  // (the call clears the pile, the kernel adds to it)
    tps::AlignArgs a{};
    a.codes = co.data(); a.length = len.data(); a.ref_codes = rco.data(); a.ref_length = rlen.data(); a.ref = rf.data(); a.centre = ce.data();
    a.pile_row = pile_row ? pr.data() : nullptr;
    a.stat = st.data();
    a.cols = cols ? cl.data() : nullptr;
    a.pile = pile ? pl.data() : nullptr;
    a.n = n;
    a.span = span; a.cdw = cdw; a.rows = tps::align_rows(length, ref, n);
    emu::WaveLds lds(tps::align_lds_dw(span, cdw, a.rows));
    for (int64_t i = 0; i < n; ++i) tps::window_align_row(a, i, lds.poisoned());
    memcpy(stat, st.data(), st.size() * 4);
    if (cols) memcpy(cols, cl.data(), cl.size() * 2);
    if (pile) memcpy(pile, pl.data(), pl.size() * 4);
    return TPS_OK;
}
