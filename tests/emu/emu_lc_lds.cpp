// TEST INFRASTRUCTURE ONLY -- the host emulation of emu_scan.cpp once more, as a library of its own, for the resident candidate
// sums of the default kernels (tests/test_lc_lds_emulation.py, tests/test_gpu_lc_lds.py):
//   * emu_set_lc_lds: PlanKnobs::lc_lds of the scans that follow (emu_scan.cpp's own library constructs PlanKnobs() and so keeps the
//     off-chip layout).  emu_set_knobs resets every knob, this one included: the driver calls emu_set_lc_lds after it;
//   * emu_counter_ext: every emulation counter of csrc/tps_wave.h (15 = sums tiles that kept their candidates in LDS);
//   * emu_plan_lc_lds: ScanArgs::lc_lds as plan_geometry decides it with the knobs of the library's contexts (tps::product_knobs).
#include "emu_scan.cpp"

extern "C" void emu_set_lc_lds(int on) { g_knobs.lc_lds = on != 0; }
extern "C" int emu_counter_ext(int i) { return (i >= 0 && i < tps::EMU_COUNTERS) ? tps::emu_counter(i) : -1; }

// out3: lc_lds, lc_cap, the entries the region of this slide holds (tps::lc_lds_entries); val_on: the batch has non-ACGT letters
extern "C" int emu_plan_lc_lds(const char* pats, int P, int k, const tps_params* prm, int64_t max_nwin, int val_on, int32_t* out3) {
    std::vector<uint32_t> lut;
    tps::ScanArgs a{};
    a.val_on = val_on ? 1 : 0;
    std::string err = tps::build_patterns(pats, P, k, lut, a.pat);
    if (err.empty()) err = tps::plan_geometry(a, *prm, k, P, max_nwin, 160 * 1024 / 4, tps::product_knobs());
    if (!err.empty()) { g_err = err; return TPS_E_CAPACITY; }
    out3[0] = a.lc_lds;
    out3[1] = a.lc_cap;
    out3[2] = a.variant ? tps::lc_lds_entries(tps::fused_seq_dw(prm->slide)) : 0;
    if (a.lc_lds && a.lc_global) { g_err = "lc_lds and lc_global both set"; return TPS_E_STATE; }
    return TPS_OK;
}
