// TEST INFRASTRUCTURE ONLY -- the host emulation of emu_scan.cpp once more, as a library of its own, with what the change-point
// tests (tests/test_binseg_paths.py) read on top of it:
//   * emu_counter_ext: every emulation counter of csrc/tps_wave.h (emu_scan.cpp exports the first eight);
//   * emu_scan_lc: one scan of a batch through the default sums kernel of slide 6 (tables without self-overlapping k-mers, a batch
//     without non-ACGT letters: scan_read<6, false, PAIR, false>), which hands back the reads' candidate-sum scratch blocks beside
//     the results -- emu_scan keeps them to itself.
#include "emu_scan.cpp"

extern "C" int emu_counter_ext(int i) { return (i >= 0 && i < tps::EMU_COUNTERS) ? tps::emu_counter(i) : -1; }

// lc_out: n blocks of lc_words 32-bit entries (the caller sizes them from the longest read: n_win / jump + 1), entries the
// kernel never wrote keep the fill 0xBEEFBEEF; *lc_cap_out = ScanArgs::lc_cap of the scan
extern "C" int emu_scan_lc(const char* pats, int P, int k, const uint8_t* bases, const int64_t* offsets, int64_t n, const tps_params* prm,
                           int lc_cap_force, tps_read_result* results, int64_t* win_off_out, int32_t* sums, uint32_t* lc_out, int64_t lc_words,
                           int32_t* lc_cap_out) {
    std::vector<uint32_t> lut;
    tps::ScanArgs a{};
    a.val_on = 0;
    std::string err = tps::build_patterns(pats, P, k, lut, a.pat);
    if (!err.empty()) { g_err = err; return TPS_E_PATTERN; }
    tps::BatchLayout lay;
    tps::plan_batch_layout(offsets, n, *prm, lay);
    const std::vector<int64_t>& win_off = lay.win_off, &win_off16 = lay.win_off16;
    memcpy(win_off_out, win_off.data(), (size_t)(n + 1) * 8);
    err = tps::plan_geometry(a, *prm, k, P, lay.max_nwin, 160 * 1024 / 4, knobs_with(0, 0));
    if (!err.empty()) { g_err = err; return TPS_E_CAPACITY; }
    if (a.variant != 6 || a.pat.so_mask != 0 || a.pair16 || a.lut16 || a.lut_fields) { g_err = "emu_scan_lc: not a default sums kernel of slide 6"; return TPS_E_ARG; }
    // (lc_cap_force: a smaller capacity than the plan's max n_win / jump + 2 -- the kernel takes a read as long as
    // n_win / jump + 1 <= lc_cap, so the tightest cap makes the longest read's last candidate the block's last entry)
    if (lc_cap_force > 0 && lc_cap_force < a.lc_cap) a.lc_cap = lc_cap_force;
    *lc_cap_out = a.lc_cap;

    const emu::Batch batch(bases, offsets, n);
    batch.set(a);
    a.lut = lut.data();
    a.results = results;
    a.win_off = win_off.data();
    a.sums = sums;
    std::vector<uint16_t> sums16((size_t)win_off16[(size_t)n] + 8, (uint16_t)0xBEEF);
    a.sums16 = sums16.data();
    a.win_off16 = win_off16.data();
    a.n_reads = n;
    a.prm = *prm;
    std::vector<uint16_t> lc_scratch((size_t)n * (size_t)a.lc_stride + 8, (uint16_t)0xBEEF);
    a.lc_scratch = lc_scratch.data();
    std::vector<uint32_t> lutbuf((size_t)a.pair_n + lut.size());
    uint32_t* lut1 = lutbuf.data() + a.pair_n;
    for (size_t i = 0; i < lut.size(); ++i) lut1[i] = (lut[i] << 16) | (uint32_t)__builtin_popcount(lut[i]);
    for (int c = 0; c < a.pair_n; ++c) {
        const uint32_t e1 = lut1[c & a.pat.kmask], e2 = lut1[(c >> 2) & a.pat.kmask];
        lutbuf[(size_t)c] = ((e1 | e2) & 0xFFFF0000u) | ((e1 + e2) & 0xFFFFu);
    }
    std::vector<uint32_t> ldsbuf((size_t)tps::lds_dwords(a) + 16);
    uint32_t* lds = (uint32_t*)(((uintptr_t)ldsbuf.data() + 15) & ~(uintptr_t)15);
    for (int64_t r = 0; r < n; ++r) {
        for (int64_t i = 0; i < tps::lds_dwords(a); ++i) lds[i] = 0xDEADBEEFu;
        if (a.pair_n) tps::scan_read<6, false, true, false>(a, r, lds, lut1);
        else tps::scan_read<6, false, false, false>(a, r, lds, lut1);
    }
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t w = 0; w < win_off[(size_t)i + 1] - win_off[(size_t)i]; ++w)
            sums[win_off[(size_t)i] + w] = (int32_t)sums16[(size_t)(win_off16[(size_t)i] + w)];
        const uint32_t* blk = (const uint32_t*)(lc_scratch.data() + (size_t)i * (size_t)a.lc_stride);
        for (int64_t c = 0; c < lc_words; ++c) lc_out[i * lc_words + c] = c < a.lc_stride / 2 ? blk[c] : 0xBEEFBEEFu;
    }
    return TPS_OK;
}
