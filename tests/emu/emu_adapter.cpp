// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the adapter kernel (adapter_read, topsicle_amd/csrc/tps_adapter.h).
//
// Like emu_anchor.cpp: the header compiled with -DTPS_EMU, the batch packed by the library's own packer, the argument checks of
// tps_batch_adapter_find (the library's own: adapter_find_check) with its return codes, the match masks built by
// the function the library calls.  Never linked into the product.  emu_adapter_main.cpp includes this file and adds a main() for the
// stand-alone sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_adapter.h"
#include "emu_batch.h"

static std::string g_err;
extern "C" const char* emu_adapter_last_error() { return g_err.c_str(); }

// tps_batch_upload + tps_batch_adapter_find.  base_shift moves the batch inside its buffer by whole quads; words the layout does not
// own are garbage.
extern "C" int emu_adapter_find(const uint8_t* bases, const int64_t* offsets, int64_t n, const uint64_t* patterns, const int32_t* pat_len, int n_pat,
                                const uint8_t* tails, const int32_t* begin, const int32_t* end, int64_t n_reads, int base_shift, uint16_t* hits,
                                int64_t hits_len) {
    tps::Why why;
    if (const int rc = tps::adapter_find_check(n, patterns, pat_len, n_pat, tails, begin, end, n_reads, hits, hits_len, &why)) { g_err = why.msg; return rc; }
    if (n == 0) return TPS_OK;
    const emu::Batch batch(bases, offsets, n, base_shift);
    // rows of exactly their sizes: a sanitizer build sees an access past them (the kernel writes every entry)
    std::vector<uint64_t> peq((size_t)n_pat * 4);
    std::vector<int32_t> lens(pat_len, pat_len + n_pat);
    tps::adapter_build_peq(patterns, pat_len, n_pat, peq.data());
    std::vector<uint32_t> out((size_t)(n * n_pat), 0xEEEEEEEEu);
    tps::AdapterArgs a{};
    batch.set(a);
    a.peq = peq.data(); a.pat_len = lens.data();
    a.tails = tails; a.begin = begin; a.end = end;
    a.hits = out.data(); a.n_reads = n; a.n_pat = n_pat;
    emu::WaveLds lds(tps::ADAPTER_LDS_DW);
    for (int64_t r = 0; r < n; ++r) tps::adapter_read(a, r, lds.poisoned());
    memcpy(hits, out.data(), out.size() * 4);
    return TPS_OK;
}
