// TEST INFRASTRUCTURE ONLY -- sequential host emulation of the end sketch and link kernels (end_sketch_read, sketch_links_row,
// topsicle_amd/csrc/tps_ends.h).
//
// Like emu_tract.cpp: the header compiled with -DTPS_EMU, the batch packed by the library's own packer, the argument checks of
// tps_batch_end_sketch and tps_sketch_links (end_sketch_check, sketch_links_check: the library's own) with their return codes,
// the hit table and the bucket-major copy built by the functions the library calls.  Never linked into the product.
// emu_ends_main.cpp includes this file and adds a main() for the stand-alone sanitizer run.
#define TPS_EMU 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../topsicle_amd/csrc/tps_ends.h"
#include "emu_batch.h"

static std::string g_err;
extern "C" const char* emu_ends_last_error() { return g_err.c_str(); }

// k-mer positions of a staged piece (the seam cases are built from it)
extern "C" int emu_ends_piece() { return tps::ENDS_PIECE; }

// tps_batch_upload + tps_batch_end_sketch.  base_shift moves the batch inside its buffer by whole quads; words the layout does not
// own are garbage.
extern "C" int emu_end_sketch(const uint8_t* bases, const int64_t* offsets, int64_t n, uint64_t unit, int m, int k, int buckets, const uint8_t* tails,
                              const int32_t* begin, const int32_t* end, int64_t n_reads, int base_shift, uint32_t* sketch, int64_t sketch_len,
                              uint32_t* kept, int64_t kept_len) {
    tps::Why why;
    if (const int rc = tps::end_sketch_check(n, unit, m, k, buckets, tails, begin, end, n_reads, sketch, sketch_len, kept, kept_len, &why)) { g_err = why.msg; return rc; }
    if (n == 0) return TPS_OK;
    const emu::Batch batch(bases, offsets, n, base_shift);
    memset(sketch, 0xEE, (size_t)sketch_len * 4);                             // (the kernel writes every entry of these two)
    memset(kept, 0xEE, (size_t)kept_len * 4);
    const int w = m < tps::TRACT_MAX_WORD ? m : tps::TRACT_MAX_WORD;
    std::vector<uint32_t> table((size_t)tps::tract_table_dw(w));              // exactly the table: a sanitizer build sees a look-up past it
    tps::tract_hit_table(unit, m, table.data());
    tps::EndSketchArgs a{};
    batch.set(a);
    a.table = table.data();
    a.tails = tails; a.begin = begin; a.end = end;
    a.sketch = sketch; a.kept = kept; a.n_reads = n;
    a.w = w; a.k = k; a.buckets = buckets; a.shift = 32 - tps::ends_log2(buckets);
    emu::WaveLds lds(tps::ENDS_LDS_DW);
    for (int64_t r = 0; r < n; ++r) tps::end_sketch_read(a, r, lds.poisoned(), a.table);
    return TPS_OK;
}

// tps_sketch_links
extern "C" int emu_sketch_links(const uint32_t* sketch, int64_t n, int buckets, int64_t sketch_len, int min_match, int max_links, int32_t* degree,
                                int64_t degree_len, int32_t* links, int64_t links_len, int32_t* matches, int64_t matches_len) {
    tps::Why why;
    if (const int rc = tps::sketch_links_check(sketch, n, buckets, sketch_len, min_match, max_links, degree, degree_len, links, links_len, matches, matches_len, &why)) {
        g_err = why.msg;
        return rc;
    }
    if (n == 0) return TPS_OK;
    std::vector<uint32_t> t((size_t)(n * buckets));                           // exactly the copy: a sanitizer build sees a load past it
    tps::links_transpose(sketch, n, buckets, t.data());
    memset(degree, 0xEE, (size_t)degree_len * 4);                             // (the kernel writes every entry)
    memset(links, 0xFF, (size_t)links_len * 4);                               // (the library's hipMemsetAsync: -1, 0)
    memset(matches, 0, (size_t)matches_len * 4);
    tps::LinkArgs a{};
    a.t = t.data(); a.degree = degree; a.links = links; a.matches = matches;
    a.n = n; a.buckets = buckets; a.min_match = min_match; a.max_links = max_links;
    std::vector<uint32_t> row((size_t)buckets);                               // exactly the row, as the sketch is long
    for (int64_t i = 0; i < n; ++i) {
        for (int b = 0; b < buckets; ++b) row[(size_t)b] = 0xDEADBEEFu;
        tps::sketch_links_row(a, i, row.data());
    }
    return TPS_OK;
}
