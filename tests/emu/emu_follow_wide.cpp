// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the wide followers kernel (followers_wide_read, topsicle_amd/csrc/tps_wide.h).
//
// Like emu_wide.cpp for the wide scan: the header compiled with -DTPS_EMU, the table built by the very function the library calls
// (tps_wide_plan.h), the argument checks of tps_batch_kmer_followers_wide restated with its return codes.  Never linked into the product.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_wide.h"
#include "../../topsicle_amd/csrc/tps_wide_plan.h"
#include "../../topsicle_amd/csrc/tps_pack.h"

static std::string g_err;
extern "C" const char* emu_follow_wide_last_error() { return g_err.c_str(); }

// tps_set_patterns_wide + tps_batch_upload + tps_batch_kmer_followers_wide: picks[n][2][n_fwd][pw], hist[2][n_fwd][4^follow + 1] or
// NULL.  base_shift moves the batch inside its buffer by whole quads; words the layout does not own are garbage.
extern "C" int emu_followers_wide(const char* pats, int P, int k, const uint8_t* bases, const int64_t* offsets, int64_t n, int n_fwd, int follow,
                                  int lo, int hi, int min_len, int base_shift, uint32_t* picks, unsigned long long* hist) {
    std::vector<uint32_t> img;
    tps::FollowWideArgs a{};
    std::string err = tps::build_wide_table(pats, P, k, img, a.pat);
    if (!err.empty()) { g_err = err; return TPS_E_PATTERN; }
    if (n_fwd < 1 || n_fwd > tps::FOLLOWW_MAX_FWD || 2 * n_fwd > P) { g_err = "n_fwd must be 1..32 and the table must hold the complements behind the k-mers"; return TPS_E_ARG; }
    if (follow < 0) { g_err = "follow must not be negative"; return TPS_E_ARG; }
    if (lo < 0 || hi <= lo || hi - lo > tps::FOLLOW_MAX_SPAN) { g_err = "the scanned range [lo, hi) must hold 1..4096 bases"; return TPS_E_CAPACITY; }
    if (hist && follow > 8) { g_err = "the followers histogram has 4^follow bins: follow must be 0..8 bases with it"; return TPS_E_CAPACITY; }
    if (tps::followers_wide_wg_lds_dwords() * 4 > 160 * 1024) { g_err = "the wide followers kernel's LDS does not fit"; return TPS_E_CAPACITY; }
    std::vector<tps_read_desc> desc((size_t)(n > 0 ? n : 1));
    const int64_t n_words = tps::pack_layout(offsets, n, desc.data());
    const int64_t lead = 4 * (int64_t)(base_shift & 3);
    std::vector<uint32_t> seq2buf((size_t)(n_words + lead + 8), 0xDEADBEEFu);
    std::vector<uint16_t> invbuf((size_t)(n_words + lead + 8), (uint16_t)0xFFFFu);
    for (int64_t i = 0; i < n; ++i) desc[(size_t)i].word_off += lead;
    tps::pack_range(bases, offsets, 0, n, desc.data(), seq2buf.data(), invbuf.data());
    a.seq2 = seq2buf.data(); a.inv = invbuf.data(); a.desc = desc.data();
    a.picks = picks; a.hist = hist; a.n_reads = n;
    a.n_fwd = n_fwd; a.follow = follow; a.lo = lo; a.hi = hi; a.min_len = min_len; a.pw = (hi - lo + 31) / 32;
    a.nbins = hist ? (1 << (2 * follow)) + 1 : 0;
    // the workgroup's copy of the table image and exactly one wave's slice, 16-byte aligned like LDS: the sanitizer build sees
    // every access past either
    uint32_t *img_al = nullptr, *lds = nullptr;
    if (posix_memalign((void**)&img_al, 16, (size_t)tps::WIDE_IMG_DW * 4) || posix_memalign((void**)&lds, 16, (size_t)tps::FOLLOWW_LDS_DW * 4)) {
        free(img_al);
        g_err = "out of memory";
        return TPS_E_ARG;
    }
    memcpy(img_al, img.data(), (size_t)tps::WIDE_IMG_DW * 4);
    a.img = img_al;
    for (int64_t r = 0; r < n; ++r) {
        for (int i = 0; i < tps::FOLLOWW_LDS_DW; ++i) lds[i] = 0xDEADBEEFu;       // LDS content is undefined at workgroup start
        tps::followers_wide_read(a, r, lds, img_al);
    }
    free(lds);
    free(img_al);
    return TPS_OK;
}
