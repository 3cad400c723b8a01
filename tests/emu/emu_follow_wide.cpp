// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the wide followers kernel (followers_wide_read, topsicle_amd/csrc/tps_wide.h).
//
// Like emu_wide.cpp for the wide scan: the header compiled with -DTPS_EMU, the table built by the very function the library calls
// (tps_wide_plan.h), the argument checks of tps_batch_kmer_followers_wide the library's own (followers_wide_check).  Never linked into the product.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_wide.h"
#include "../../topsicle_amd/csrc/tps_wide_plan.h"
#include "emu_batch.h"

static std::string g_err;
extern "C" const char* emu_follow_wide_last_error() { return g_err.c_str(); }

// tps_set_patterns_wide + tps_batch_upload + tps_batch_kmer_followers_wide: picks[n][2][n_fwd][pw], hist[2][n_fwd][4^follow + 1] or
// NULL.  base_shift moves the batch inside its buffer by whole quads; words the layout does not own are garbage.
extern "C" int emu_followers_wide(const char* pats, int P, int k, const uint8_t* bases, const int64_t* offsets, int64_t n, int n_fwd, int follow,
                                  int lo, int hi, int min_len, int base_shift, uint32_t* picks, int64_t picks_words, unsigned long long* hist,
                                  int64_t hist_len) {
    std::vector<uint32_t> img;
    tps::FollowWideArgs a{};
    std::string err = tps::build_wide_table(pats, P, k, img, a.pat);
    if (!err.empty()) { g_err = err; return TPS_E_PATTERN; }
    tps::Why why;
    if (const int rc = tps::followers_wide_check(P, n, n_fwd, follow, lo, hi, picks, picks_words, hist, hist_len, &why)) { g_err = why.msg; return rc; }
    const emu::Batch batch(bases, offsets, n, base_shift);
    batch.set(a);
    a.picks = picks; a.hist = hist; a.n_reads = n;
    a.n_fwd = n_fwd; a.follow = follow; a.lo = lo; a.hi = hi; a.min_len = min_len; a.pw = (hi - lo + 31) / 32;
    a.nbins = hist ? (1 << (2 * follow)) + 1 : 0;
    // the workgroup's copy of the table image and exactly one wave's slice, 16-byte aligned like LDS: the sanitizer build sees
    // every access past either
    emu::WaveLds img_al(tps::WIDE_IMG_DW), lds(tps::FOLLOWW_LDS_DW);
    memcpy(img_al.p, img.data(), (size_t)tps::WIDE_IMG_DW * 4);
    a.img = img_al.p;
    for (int64_t r = 0; r < n; ++r) tps::followers_wide_read(a, r, lds.poisoned(), img_al.p);
    return TPS_OK;
}
