// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the window and offset kernels (end_window_read, window_offsets_row,
// topsicle_amd/csrc/tps_anchor.h).
//
// Like emu_ends.cpp: the header compiled with -DTPS_EMU, the batch packed by the library's own packer, the argument checks of
// tps_batch_end_window and tps_window_offsets (the library's own: end_window_check,
// window_offsets_check) with their return codes, the hit table built by the function the library
// calls.  Never linked into the product.  emu_anchor_main.cpp includes this file and adds a main() for the stand-alone sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_anchor.h"
#include "emu_batch.h"

static std::string g_err;
extern "C" const char* emu_anchor_last_error() { return g_err.c_str(); }

// tps_batch_upload + tps_batch_end_window.  base_shift moves the batch inside its buffer by whole quads; words the layout does not
// own are garbage.
extern "C" int emu_end_window(const uint8_t* bases, const int64_t* offsets, int64_t n, uint64_t unit, int m, int k, const uint8_t* tails, const int32_t* begin,
                              const int32_t* end, int64_t n_reads, int span, int base_shift, uint32_t* codes, int64_t codes_len, uint32_t* keep,
                              int64_t keep_len) {
    tps::Why why;
    if (const int rc = tps::end_window_check(n, unit, m, k, tails, begin, end, n_reads, span, codes, codes_len, keep, keep_len, &why)) { g_err = why.msg; return rc; }
    if (n == 0) return TPS_OK;
    const int cdw = (span + 15) / 16, kdw = (span + 31) / 32;
    const emu::Batch batch(bases, offsets, n, base_shift);
    // exactly the rows: a sanitizer build sees a store past them (the kernel writes every entry)
    std::vector<uint32_t> co((size_t)codes_len, 0xEEEEEEEEu), kp((size_t)keep_len, 0xEEEEEEEEu);
    const int w = m < tps::TRACT_MAX_WORD ? m : tps::TRACT_MAX_WORD;
    std::vector<uint32_t> table((size_t)tps::tract_table_dw(w));
    tps::tract_hit_table(unit, m, table.data());
    tps::EndWindowArgs a{};
    batch.set(a);
    a.table = table.data();
    a.tails = tails; a.begin = begin; a.end = end;
    a.codes = co.data(); a.keep = kp.data(); a.n_reads = n;
    a.w = w; a.k = k; a.cdw = cdw; a.kdw = kdw;
    emu::WaveLds lds(tps::ENDS_LDS_DW);
    for (int64_t r = 0; r < n; ++r) tps::end_window_read(a, r, lds.poisoned(), a.table);
    memcpy(codes, co.data(), co.size() * 4);
    memcpy(keep, kp.data(), kp.size() * 4);
    return TPS_OK;
}

// tps_window_offsets
extern "C" int emu_window_offsets(const uint32_t* codes, const uint32_t* keep, const int32_t* length, const int32_t* ref, int64_t n, int span, int k,
                                  int32_t* offset, int32_t* votes, int32_t* second, int64_t out_len) {
    tps::Why why;
    if (const int rc = tps::window_offsets_check(codes, keep, length, ref, n, span, k, offset, votes, second, out_len, &why)) { g_err = why.msg; return rc; }
    if (n == 0) return TPS_OK;
    const int cdw = (span + 15) / 16, kdw = (span + 31) / 32;
    // exactly the rows, as the device buffers are long: a sanitizer build sees a load past them
    std::vector<uint32_t> co(codes, codes + n * cdw), kp(keep, keep + n * kdw);
    std::vector<int32_t> out((size_t)(3 * n), (int32_t)0xEEEEEEEE);             // (the kernel writes every entry)
    tps::OffsetArgs a{};
    a.codes = co.data(); a.keep = kp.data(); a.length = length; a.ref = ref;
    a.offset = out.data(); a.votes = out.data() + n; a.second = out.data() + 2 * n;
    a.n = n; a.k = k; a.cdw = cdw; a.kdw = kdw;
    emu::WaveLds lds(tps::OFFSETS_LDS_DW);
    for (int64_t i = 0; i < n; ++i) tps::window_offsets_row(a, i, lds.poisoned());
    memcpy(offset, a.offset, (size_t)n * 4);
    memcpy(votes, a.votes, (size_t)n * 4);
    memcpy(second, a.second, (size_t)n * 4);
    return TPS_OK;
}
