// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the motif census kernel (motif_read, topsicle_amd/csrc/tps_motif.h).
//
// Like emu_follow_wide.cpp: the header compiled with -DTPS_EMU, the batch packed by the library's own packer, the argument checks of
// tps_batch_motif_census restated with its return codes.  Never linked into the product.  emu_motif_main.cpp includes this file and
// adds a main() for the stand-alone sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_motif.h"
#include "../../topsicle_amd/csrc/tps_pack.h"

static std::string g_err;
extern "C" const char* emu_motif_last_error() { return g_err.c_str(); }

// tps_batch_upload + tps_batch_motif_census: hits[n][2], counts[n][2][u_max - u_min + 1] or NULL.  base_shift moves the batch inside
// its buffer by whole quads; words the layout does not own are garbage.
extern "C" int emu_motif_census(const uint8_t* bases, const int64_t* offsets, int64_t n, int u_min, int u_max, int lo, int hi, int min_len,
                                int base_shift, tps_motif_hit* hits, int64_t n_hits, int32_t* counts, int64_t counts_len) {
    if (u_min < 1 || u_max < u_min || u_max > tps::MOTIF_MAX_PERIOD) { g_err = "the periods must be 1 <= u_min <= u_max <= 32"; return TPS_E_ARG; }
    if (lo < 0 || hi <= lo || hi - lo > tps::FOLLOW_MAX_SPAN) { g_err = "the scanned range [lo, hi) must hold 1..4096 bases"; return TPS_E_CAPACITY; }
    const int nu = u_max - u_min + 1;
    if ((!hits && n > 0) || n_hits != 2 * n) { g_err = "hits must hold 2 n entries"; return TPS_E_ARG; }
    if (counts && counts_len != 2 * n * nu) { g_err = "counts must hold 2 n (u_max - u_min + 1) counters"; return TPS_E_ARG; }
    if (n == 0) return TPS_OK;
    std::vector<tps_read_desc> desc((size_t)n);
    const int64_t n_words = tps::pack_layout(offsets, n, desc.data());
    const int64_t lead = 4 * (int64_t)(base_shift & 3);
    std::vector<uint32_t> seq2buf((size_t)(n_words + lead + 8), 0xDEADBEEFu);
    std::vector<uint16_t> invbuf((size_t)(n_words + lead + 8), (uint16_t)0xFFFFu);
    for (int64_t i = 0; i < n; ++i) desc[(size_t)i].word_off += lead;
    tps::pack_range(bases, offsets, 0, n, desc.data(), seq2buf.data(), invbuf.data());
    memset(hits, 0, (size_t)n_hits * sizeof(tps_motif_hit));                  // (the library's hipMemsetAsync)
    if (counts) memset(counts, 0, (size_t)counts_len * 4);
    tps::MotifArgs a{};
    a.seq2 = seq2buf.data(); a.inv = invbuf.data(); a.desc = desc.data();
    a.hits = hits; a.counts = counts; a.n_reads = n;
    a.u_min = u_min; a.u_max = u_max; a.lo = lo; a.hi = hi; a.min_len = min_len;
    // exactly one wave's slice, 16-byte aligned like LDS: a sanitizer build sees every access past it
    uint32_t* lds = nullptr;
    if (posix_memalign((void**)&lds, 16, (size_t)tps::MOTIF_LDS_DW * 4)) { g_err = "out of memory"; return TPS_E_ARG; }
    for (int64_t r = 0; r < n; ++r) {
        for (int i = 0; i < tps::MOTIF_LDS_DW; ++i) lds[i] = 0xDEADBEEFu;       // LDS content is undefined at workgroup start
        tps::motif_read(a, r, lds);
    }
    free(lds);
    return TPS_OK;
}
