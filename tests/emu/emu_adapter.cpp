// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the adapter kernel (adapter_read, topsicle_amd/csrc/tps_adapter.h).
//
// Like emu_anchor.cpp: the header compiled with -DTPS_EMU, the batch packed by the library's own packer, the argument checks of
// tps_batch_adapter_find (the library's own: adapter_check, adapter_check_reads) with their return codes, the match masks built by
// the function the library calls.  Never linked into the product.  emu_adapter_main.cpp includes this file and adds a main() for the
// stand-alone sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_adapter.h"
#include "../../topsicle_amd/csrc/tps_pack.h"

static std::string g_err;
extern "C" const char* emu_adapter_last_error() { return g_err.c_str(); }

// tps_batch_upload + tps_batch_adapter_find.  base_shift moves the batch inside its buffer by whole quads; words the layout does not
// own are garbage.
extern "C" int emu_adapter_find(const uint8_t* bases, const int64_t* offsets, int64_t n, const uint64_t* patterns, const int32_t* pat_len, int n_pat,
                                const uint8_t* tails, const int32_t* begin, const int32_t* end, int64_t n_reads, int base_shift, uint16_t* hits,
                                int64_t hits_len) {
    const char* why = "";
    int pat_at = 0;
    int rc = tps::adapter_check(patterns, pat_len, n_pat, &why, &pat_at);
    if (rc) { g_err = why; return rc; }
    if (n_reads != n || hits_len != n * n_pat * 2) { g_err = "an array does not match the slot"; return TPS_E_ARG; }
    if (n == 0) return TPS_OK;
    if (!tails || !begin || !end || !hits) { g_err = "null array"; return TPS_E_ARG; }
    int64_t at = 0;
    if ((rc = tps::adapter_check_reads(tails, begin, end, n, &why, &at))) { g_err = why; return rc; }
    std::vector<tps_read_desc> desc((size_t)n);
    const int64_t n_words = tps::pack_layout(offsets, n, desc.data());
    const int64_t lead = 4 * (int64_t)(base_shift & 3);
    std::vector<uint32_t> seq2buf((size_t)(n_words + lead + 8), 0xDEADBEEFu);
    std::vector<uint16_t> invbuf((size_t)(n_words + lead + 8), (uint16_t)0xFFFFu);
    for (int64_t i = 0; i < n; ++i) desc[(size_t)i].word_off += lead;
    tps::pack_range(bases, offsets, 0, n, desc.data(), seq2buf.data(), invbuf.data());
    // rows of exactly their sizes: a sanitizer build sees an access past them (the kernel writes every entry)
    std::vector<uint64_t> peq((size_t)n_pat * 4);
    std::vector<int32_t> lens(pat_len, pat_len + n_pat);
    tps::adapter_build_peq(patterns, pat_len, n_pat, peq.data());
    std::vector<uint32_t> out((size_t)(n * n_pat), 0xEEEEEEEEu);
    tps::AdapterArgs a{};
    a.seq2 = seq2buf.data(); a.inv = invbuf.data(); a.desc = desc.data();
    a.peq = peq.data(); a.pat_len = lens.data();
    a.tails = tails; a.begin = begin; a.end = end;
    a.hits = out.data(); a.n_reads = n; a.n_pat = n_pat;
    // the staging area of exactly one wave's size, poisoned: LDS content is undefined at workgroup start
    std::vector<uint32_t> wave((size_t)tps::ADAPTER_LDS_DW);
    for (int64_t r = 0; r < n; ++r) {
        for (int i = 0; i < tps::ADAPTER_LDS_DW; ++i) wave[(size_t)i] = 0xDEADBEEFu;
        tps::adapter_read(a, r, wave.data());
    }
    memcpy(hits, out.data(), out.size() * 4);
    return TPS_OK;
}
