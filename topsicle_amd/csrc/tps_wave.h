// tps_wave.h -- the platform layer of the scan kernels: everything that differs between the device build (gfx950) and the
// sequential host emulation (tests/emu, -DTPS_EMU).  tps_device.h and tps_wide.h are written against it and hold ONE kernel
// text: both builds compile the same statements, so the CPU tests check the algorithm the GPU runs.
//
// The model.  One wave (NT = 64 lanes) owns one read.  A kernel is a sequence of
//   * phases     TPS_PHASE { ... tid ... }   the body runs once per lane.  Device: every lane executes it, tid is a fresh opaque
//                copy of the lane id.  Emulation: a loop over tid = 0 .. NT - 1, so phases run in program order and a phase
//                sees everything the earlier ones wrote -- which is what TPS_SYNC() guarantees on the device;
//   * wave code  between the phases: wave-uniform values, and the wave operations below.
// What a lane keeps in registers from one phase to a later one is declared as Lane<T> / LaneArr<T, N> and written TPS_AT(x) /
// TPS_AT(x)[j] where a `tid` is in scope: on the device Lane<T> IS T and LaneArr<T, N> IS T[N] (alias templates: the compiler
// sees the very declarations a device-only kernel would hold, TPS_AT(x) is x), in the emulation one T / T[N] per lane.  A plain local variable declared outside a phase is ONE variable for the whole wave in the emulation:
// it may only hold wave-uniform values.
// The wave operations (ballot of a flag, wave sums and maxima, reads of another lane's value) take such per-lane state -- computed
// from other per-lane state in a TPS_LANES block where needed; each has a device body (the intrinsic sequence) and an emulation
// body (a loop over the lanes).
// The emulation is test infrastructure only; the product library contains device code only.
#pragma once
#include <stdint.h>

#ifdef TPS_EMU
#define TPS_DEV static inline
#define TPS_HD static inline
#define TPS_AT(x) ((x).v[tid])                    // this lane's copy of per-lane state (Lane<> / LaneArr<>, below)
#define TPS_PHASE for (int tid = 0; tid < tps::NT; ++tid)
#define TPS_LANES for (int tid = 0; tid < tps::NT; ++tid)
#define TPS_PHASE_WITH(ln) for (int tid = (ln) * 0; tid < tps::NT; ++tid)
#define TPS_SYNC() ((void)0)
#define TPS_FENCE_WG() ((void)0)
#define TPS_UNROLL
#define TPS_NOVEC
#define TPS_PIN_S(x) ((void)0)
#define TPS_PIN_V(x) ((void)0)
#else
#define TPS_DEV __device__ __forceinline__
#define TPS_HD __host__ __device__ inline
#define TPS_AT(x) (x)
// Every phase gets a FRESH, opaque copy of the lane id (an empty asm the optimiser cannot see through).
// Without it LLVM hoists all lane-dependent address arithmetic of every phase out of the tile loop
// and keeps it live across the whole kernel: measured 99 -> 42 VGPRs on the fused tile alone.
__device__ __forceinline__ int tps_fresh_lane() {
    int t = (int)(threadIdx.x & 63u);
    asm volatile("" : "+v"(t));
    return t;
}
#define TPS_PHASE for (int tid = tps_fresh_lane(), once_ = 1; once_; once_ = 0)
// per-lane statements BETWEEN the phases (a lane total's exclusive prefix, a correction added to a lane's registers ...): tid is
// the plain lane id, no new opaque copy -- code that only touches Lane<> state costs nothing for it
#define TPS_LANES for (int tid = (int)(threadIdx.x & 63u), once_ = 1; once_; once_ = 0)
// a phase inside a wave-uniform loop that runs on ONE opaque lane id taken before the loop: const int ln = tps_fresh_lane();
#define TPS_PHASE_WITH(ln) if (const int tid = (ln); true)
// wave-level synchronisation: a wave's LDS operations execute in issue order, so making earlier LDS
// writes visible to the other lanes of the SAME wave only needs the compiler not to reorder / cache
// across this point (no s_barrier, no cross-wave skew)
#define TPS_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
// same wave, same CU: workgroup scope orders this wave's own global stores before its own later loads / byte updates (an
// agent-scope fence writes the L2 back: measured 5x slower)
#define TPS_FENCE_WG() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup")
#define TPS_UNROLL _Pragma("unroll")
// short runtime-bounded loops: keep them as plain scalar loops (the vectoriser turns a 1-2 iteration loop
// into prologue / vector body / epilogue control flow that costs more than the loop)
#define TPS_NOVEC _Pragma("clang loop vectorize(disable) interleave(disable) unroll(disable)")
// (__builtin_amdgcn_sched_barrier(0) was used here to bound register pressure; with ROCm 7.2 it made the
// self-overlap + invalid-base instance of the fused tile nondeterministic on gfx950, and it is no longer
// needed once every phase launders its lane id)
// zero-cost "redefinition" of a wave-uniform value: it stays in an SGPR (or a VGPR lane) instead of being re-loaded from the
// kernel-argument segment inside a loop (an s_load + s_waitcnt that also drains the LDS queue)
#define TPS_PIN_S(x) asm volatile("" : "+s"(x))
// the same for a per-lane value: it is computed HERE (the compiler otherwise sinks pure arithmetic past the wave barrier
// of the next phase and keeps all its inputs alive across it)
#define TPS_PIN_V(x) asm volatile("" : "+v"(x))
#endif

// diagnostics: thread 0 stores the shader clock at phase boundaries when ScanArgs::stamps is set
// (TPS_ISA_MARKS, scripts/isa_budget.py: the same boundaries and the phases of the sums tiles as comments in the ISA -- a static
// instruction budget per phase; never in the product library)
#if defined(TPS_ISA_MARKS) && !defined(TPS_EMU)
#define TPS_STAMP(i) asm volatile(";tps_stamp %0" ::"i"(i))
#define TPS_ISA_MARK(id) asm volatile(";tps_mark %0" ::"i"(id))
#define TPS_ISA_REGION(id) asm volatile(";tps_region %0" ::"i"(id))
#elif defined(TPS_EMU) || !defined(TPS_STAMPS)
#define TPS_STAMP(i) ((void)0)
#define TPS_ISA_MARK(id) ((void)(id))
#define TPS_ISA_REGION(id) ((void)(id))
#else
#define TPS_STAMP(i) do { if (a.stamps && (threadIdx.x & 63u) == 0) a.stamps[r * 16 + (i)] = __builtin_readcyclecounter(); } while (0)
#define TPS_ISA_MARK(id) ((void)(id))
#define TPS_ISA_REGION(id) ((void)(id))
#endif
// (TPS_ISA_REGION: the parts of a read's program OUTSIDE the tile phases, for the same static budget -- 1 tile set-up, 2 the
// tile's staging store, 3 the next tile's prefetch, 4 the tile dispatch, 5 the change point's float32 prefilter, 8 its one-lane
// finish, 6 its float64 stage of every lane and the wave reduction, 7 the exact tournament and the result, 9 step 1 of the
// pair-table kernels (trc_decide_pairs))
// ... inside the per-pattern tiles (first tile of a read only): 6 = phase 1 done, 7 = windows done, 11 = rows out, 12 = candidates done
#if defined(TPS_EMU) || !defined(TPS_STAMPS)
#define TPS_PP_STAMP(i) ((void)0)
#else
#define TPS_PP_STAMP(i) do { if (w0 == 0 && a.stamps && (threadIdx.x & 63u) == 0) a.stamps[tc.rd * 16 + (i)] = __builtin_readcyclecounter(); } while (0)
#endif

namespace tps {

constexpr int NT = 64;                            // lanes that cooperate on one read: one wave

// counters the tests read (emulation only; the numbering is the tests'): 0 = per-pattern tiles, 1 = windows recounted there,
// 2 = lanes of a per-pattern tile whose look-back could not fix their state, 3 = sums tiles with the window phase in 16-bit pairs
// (and chain-parity repairs of the per-pattern tiles), 4 = exact change-point tournaments, 5 = sums tiles of a self-overlap
// table with chains corrected, 6 = ... without a chain, 7 = sums tiles that store their candidates lane by lane, 8 = change points
// finished by the one lane whose candidate passed the prefilter, 9 = ... by the float64 stage of every lane and the wave reduction,
// 10 = prefilters that found a lane with two candidates inside the margin (crowded), 11 = prefilters run on the float64 D route,
// the route a read's step 1 took: 12 = trc_decide_pairs, 13 = the packed counts (trc_count_packed; the device's
// trc_decide_packed among them), 14 = the histograms (trc_count_thread); 15 = sums tiles that keep their candidates in LDS
// (ScanArgs::lc_lds: a subset of 7)
#ifdef TPS_EMU
constexpr int EMU_COUNTERS = 16;
inline int& emu_counter(int i) { static int c[EMU_COUNTERS] = {0}; return c[i]; }
#define TPS_EMU_COUNT(i) ((void)++tps::emu_counter(i))
#define TPS_EMU_COUNT_N(i, n) ((void)(tps::emu_counter(i) += (int)(n)))
TPS_DEV int tps_fresh_lane() { return 0; }
#else
#define TPS_EMU_COUNT(i) ((void)0)
#define TPS_EMU_COUNT_N(i, n) ((void)0)
#endif

// ------------------------------------------------------------------ per-lane state that outlives a phase
#ifdef TPS_EMU
template <typename T>
struct Lane {
    T v[NT];
    Lane() {}
    Lane(T x) { for (int t = 0; t < NT; ++t) v[t] = x; }
};
template <typename T, int N>
struct LaneArr {
    T v[NT][N];
};
#else
template <typename T> using Lane = T;
template <typename T, int N> using LaneArr = T[N];
#endif

// ------------------------------------------------------------------ wave operations (between the phases unless said otherwise)
// the lanes whose flag is set, as a 64-bit mask (any: != 0, count: popcount)
#ifdef TPS_EMU
TPS_DEV uint64_t wave_ballot(const Lane<bool>& p) {
    uint64_t m = 0;
    for (int t = 0; t < NT; ++t) m |= (uint64_t)(p.v[t] ? 1 : 0) << t;
    return m;
}
#else
TPS_DEV uint64_t wave_ballot(const Lane<bool>& p) { return __builtin_amdgcn_ballot_w64(p); }
#endif
// inside a phase: how many of the lanes 0 .. tid have their bit set in the ballot `b` (wave-uniform).  Device: the two v_mbcnt count
// the bits below the lane; shifted down by one they cover bits 1 .. tid, and bit 0 goes in as the scalar start value.
#ifdef TPS_EMU
TPS_DEV int wave_ballot_upto(uint64_t b, int tid) { return __builtin_popcountll(tid >= NT - 1 ? b : b & ((2ull << tid) - 1ull)); }
#else
TPS_DEV int wave_ballot_upto(uint64_t b, int tid) {
    (void)tid;
    const uint64_t s = b >> 1;
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(s >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)s, (uint32_t)(b & 1ull)));
}
#endif
// inclusive prefix sum over the lanes (device: DPP row shifts / broadcasts, six VALU adds, no LDS round trips)
#ifdef TPS_EMU
TPS_DEV Lane<uint32_t> wave_incl_sum(const Lane<uint32_t>& x) {
    Lane<uint32_t> r;
    uint32_t acc = 0;
    for (int t = 0; t < NT; ++t) { acc += x.v[t]; r.v[t] = acc; }
    return r;
}
TPS_DEV Lane<uint32_t> wave_excl_sum(const Lane<uint32_t>& x) {
    Lane<uint32_t> r;
    uint32_t acc = 0;
    for (int t = 0; t < NT; ++t) { r.v[t] = acc; acc += x.v[t]; }
    return r;
}
#else
TPS_DEV Lane<uint32_t> wave_incl_sum(const Lane<uint32_t>& x) {
    uint32_t inc = x;
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x111, 0xf, 0xf, false);   // row_shr:1
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x112, 0xf, 0xf, false);   // row_shr:2
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x114, 0xf, 0xf, false);   // row_shr:4
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x118, 0xf, 0xf, false);   // row_shr:8
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return inc;
}
TPS_DEV Lane<uint32_t> wave_excl_sum(const Lane<uint32_t>& x) { return wave_incl_sum(x) - x; }
#endif
// wave-wide maximum of an unsigned value (device: DPP, no LDS round trip)
#ifdef TPS_EMU
TPS_DEV uint32_t wave_max_u32(const Lane<uint32_t>& x) {
    uint32_t m = 0;
    for (int t = 0; t < NT; ++t) m = x.v[t] > m ? x.v[t] : m;
    return m;
}
#else
TPS_DEV uint32_t wave_max_u32(const Lane<uint32_t>& x) {
    uint32_t v = x;
    auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
#endif
// inclusive prefix minimum over the lanes: lane l gets the smallest x of lanes 0 .. l (device: the DPP steps of wave_incl_sum; a lane
// a shift or a broadcast does not reach takes the `old` operand, the minimum's identity)
#ifdef TPS_EMU
TPS_DEV Lane<uint32_t> wave_incl_min_u32(const Lane<uint32_t>& x) {
    Lane<uint32_t> r;
    uint32_t acc = 0xFFFFFFFFu;
    for (int t = 0; t < NT; ++t) { acc = x.v[t] < acc ? x.v[t] : acc; r.v[t] = acc; }
    return r;
}
#else
TPS_DEV Lane<uint32_t> wave_incl_min_u32(const Lane<uint32_t>& x) {
    uint32_t v = x;
    auto mn = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
    v = mn(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = mn(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = mn(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = mn(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = mn(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast:15 -> rows 1, 3
    v = mn(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast:31 -> rows 2, 3
    return v;
}
#endif
// the sums of a per-lane value over lanes 0 .. 31 (lo) and over lanes 32 .. 63 (hi), both wave-uniform (device: DPP row sums, the
// rows' totals broadcast into the next row, lanes 31 and 63 read)
#ifdef TPS_EMU
TPS_DEV void wave_half_sums(const Lane<uint32_t>& x, uint32_t& lo, uint32_t& hi) {
    lo = hi = 0;
    for (int t = 0; t < NT / 2; ++t) { lo += x.v[t]; hi += x.v[t + NT / 2]; }
}
#else
TPS_DEV void wave_half_sums(const Lane<uint32_t>& x, uint32_t& lo, uint32_t& hi) {
    uint32_t v = x;
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    lo = (uint32_t)__builtin_amdgcn_readlane((int)v, 31);
    hi = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
#endif
// the value lane `src` holds: src wave-uniform (v_readlane) / src per lane, inside a phase (ds_bpermute)
#ifdef TPS_EMU
TPS_DEV uint32_t wave_read_lane(const Lane<uint32_t>& x, int src) { return x.v[src]; }
TPS_DEV int wave_read_lane(const Lane<int>& x, int src) { return x.v[src]; }
TPS_DEV uint32_t wave_shuffle(const Lane<uint32_t>& x, int tid, int src) { (void)tid; return x.v[src]; }
#else
TPS_DEV uint32_t wave_read_lane(const Lane<uint32_t>& x, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)x, src); }
TPS_DEV int wave_read_lane(const Lane<int>& x, int src) { return __builtin_amdgcn_readlane(x, src); }
TPS_DEV uint32_t wave_shuffle(const Lane<uint32_t>& x, int tid, int src) { (void)tid; return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)x); }
#endif

// ------------------------------------------------------------------ instructions
#ifdef TPS_EMU
TPS_DEV uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) {
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (sh & 31));
}
TPS_DEV uint32_t udot4(uint32_t a, uint32_t b) {
    uint32_t s = 0;
    for (int i = 0; i < 4; ++i) s += ((a >> (8 * i)) & 255u) * ((b >> (8 * i)) & 255u);
    return s;
}
TPS_DEV uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) {
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) {
        uint32_t c = (sel >> (8 * i)) & 255u, byte;
        if (c < 4) byte = (s1 >> (8 * c)) & 255u;
        else if (c < 8) byte = (s0 >> (8 * (c - 4))) & 255u;
        else byte = (c >= 13) ? 255u : 0u;
        out |= byte << (8 * i);
    }
    return out;
}
TPS_DEV int popc(uint32_t x) { return __builtin_popcount(x); }
TPS_DEV int ffs0(uint32_t x) { return __builtin_ctz(x); }
TPS_DEV uint32_t uniform(uint32_t x) { return x; }
TPS_DEV float rcp_f32(float x) { return 1.0f / x; }
TPS_DEV float med3_f32(float a, float b, float c) {
    const float lo = a < b ? a : b, hi = a < b ? b : a;
    return c < lo ? lo : (c > hi ? hi : c);
}
TPS_DEV void lds_add(uint32_t* p, uint32_t v) { *p += v; }
TPS_DEV void lds_or(uint32_t* p, uint32_t v) { *p |= v; }
TPS_DEV uint32_t lds_add_ret(uint32_t* p, uint32_t v) { uint32_t o = *p; *p += v; return o; }
TPS_DEV void lds_max_u64(uint64_t* p, uint64_t v) { if (v > *p) *p = v; }
TPS_DEV void lds_max_i32(int32_t* p, int32_t v) { if (v > *p) *p = v; }
TPS_DEV void lds_min_u32(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
TPS_DEV void hist_add(unsigned long long* p) { *p += 1ull; }
TPS_DEV void hist_add_n(unsigned long long* p, uint32_t v) { *p += v; }
TPS_DEV void g_add_i32(int32_t* p, int32_t v) { *p += v; }
struct u32x4 { uint32_t x, y, z, w; };
struct u32x2 { uint32_t x, y; };
TPS_DEV u32x4 load16(const uint8_t* p) { return *(const u32x4*)p; }
TPS_DEV u32x2 load8(const uint8_t* p) { return *(const u32x2*)p; }
TPS_DEV uint32_t bitrev32(uint32_t x) {
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    return __builtin_bswap32(x);
}
#else
TPS_DEV uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbit(hi, lo, sh); }
TPS_DEV uint32_t udot4(uint32_t a, uint32_t b) { return __builtin_amdgcn_udot4(a, b, 0u, false); }
TPS_DEV uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) { return __builtin_amdgcn_perm(s0, s1, sel); }
TPS_DEV int popc(uint32_t x) { return __builtin_popcount(x); }
TPS_DEV int ffs0(uint32_t x) { return __builtin_ctz(x); }
// a value every lane of the wave agrees on (e.g. read from LDS): tell the compiler it is scalar
TPS_DEV uint32_t uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
TPS_DEV float rcp_f32(float x) { return __builtin_amdgcn_rcpf(x); }      // v_rcp_f32 (1 ulp)
// the median of three numbers (none a NaN): v_med3_f32
TPS_DEV float med3_f32(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }
TPS_DEV void lds_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
TPS_DEV void lds_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
TPS_DEV uint32_t lds_add_ret(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
TPS_DEV void lds_max_u64(uint64_t* p, uint64_t v) { atomicMax((unsigned long long*)p, (unsigned long long)v); }
TPS_DEV void lds_max_i32(int32_t* p, int32_t v) { atomicMax(p, v); }
TPS_DEV void lds_min_u32(uint32_t* p, uint32_t v) { atomicMin(p, v); }
TPS_DEV void hist_add(unsigned long long* p) { atomicAdd(p, 1ull); }
TPS_DEV void hist_add_n(unsigned long long* p, uint32_t v) { atomicAdd(p, (unsigned long long)v); }
TPS_DEV void g_add_i32(int32_t* p, int32_t v) { atomicAdd(p, v); }      // a 32-bit count in global memory
typedef uint4 u32x4;
typedef uint2 u32x2;
// 16-byte load that is KNOWN to hit global memory: the address was rebuilt from an integer (aligned
// down), which makes the compiler fall back to FLAT loads -- those also count on lgkmcnt and would
// stall every LDS wait behind the prefetch.  An explicit global address space keeps them on vmcnt.
TPS_DEV u32x4 load16(const uint8_t* p) {
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) v4u* gptr_t;
    const v4u t = *(gptr_t)(uintptr_t)p;
    u32x4 r;
    r.x = t.x; r.y = t.y; r.z = t.z; r.w = t.w;
    return r;
}
TPS_DEV u32x2 load8(const uint8_t* p) {
    typedef unsigned int v2u __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(1))) v2u* gptr_t;
    const v2u t = *(gptr_t)(uintptr_t)p;
    u32x2 r;
    r.x = t.x; r.y = t.y;
    return r;
}
TPS_DEV uint32_t bitrev32(uint32_t x) { return __builtin_bitreverse32(x); }      // v_bfrev_b32
#endif

// inside a phase: every lane offers a 64-bit value (a non-negative f64 as its bit pattern), the maximum lands in *slot (LDS,
// pre-zeroed).  Device: a wave-level butterfly first, so that only one LDS atomic per wave is issued.
#ifdef TPS_EMU
TPS_DEV void wg_max_bits(uint64_t bits, uint64_t* slot) { lds_max_u64(slot, bits); }
#else
TPS_DEV void wg_max_bits(uint64_t bits, uint64_t* slot) {
    TPS_UNROLL
    for (int d = 32; d >= 1; d >>= 1) {
        uint32_t lo = __shfl_xor((uint32_t)bits, d), hi = __shfl_xor((uint32_t)(bits >> 32), d);
        uint64_t o = ((uint64_t)hi << 32) | lo;
        bits = o > bits ? o : bits;
    }
    if ((threadIdx.x & 63) != 0) return;
    lds_max_u64(slot, bits);
}
#endif

// table entry at byte offset `off` (already masked to the table size).  The table starts at the
// workgroup's LDS offset 0, i.e. it is aligned to any power of two, so base | off == base + off and the
// mask + base fold into one v_and_or_b32 -- where the base is a known 0 (every kernel's first table) into one v_and; with mask and
// base both in SGPRs (the single table of the pair-table kernels: 8 lookups per tile at odd r, step 1's) it comes out as v_and +
// v_or, a VOP3 instruction reading one scalar register only on gfx9.  The base pinned into a VGPR gives the one instruction, 6 VALU
// per tile less -- and measures nothing at config 2 (55.0 / 54.8 against 54.8 / 55.0 us), +1 % on the kernels whose base is 0: not kept.
// Nor does a compile-time table address help (tried: a fixed-size pair region, so that the single table starts at LDS byte 4096): the
// base of the dynamic LDS array is resolved after instruction selection -- `| base` of the array's own start is folded late, any
// other constant offset stays an instruction, and written as `+` even the start costs a `v_add_u32 0` per lookup.
#ifdef TPS_EMU
TPS_DEV uint32_t lut_at(const uint32_t* lut, uint32_t v4, uint32_t amask) { return *(const uint32_t*)((const char*)lut + (v4 & amask)); }
#else
TPS_DEV uint32_t lut_at(const uint32_t* lut, uint32_t v4, uint32_t amask) {
    typedef const __attribute__((address_space(3))) uint32_t* lptr_t;
    const uint32_t base = (uint32_t)(uintptr_t)(lptr_t)lut;
    return *(lptr_t)(uintptr_t)((v4 & amask) | base);
}
#endif

// 16-bit table entry (LUT_M16 tables: one pattern mask per k-mer code) at byte offset `off2` (already masked to the table size)
#ifdef TPS_EMU
TPS_DEV uint32_t lut16_at(const uint32_t* lut, uint32_t v2, uint32_t amask1) { return *(const uint16_t*)((const char*)lut + (v2 & amask1)); }
#define lut16_at_wide lut16_at
#else
TPS_DEV uint32_t lut16_at(const uint32_t* lut, uint32_t v2, uint32_t amask1) {
    typedef const __attribute__((address_space(3))) uint16_t* lptr16_t;
    const uint32_t base = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t*)lut;
    return *(lptr16_t)(uintptr_t)((v2 & amask1) | base);      // ds_read_u16: zero-extended
}
// ... for the sums tiles of the self-overlap tables (tile_lc_s<.., CD>), opaque to the optimiser: it otherwise narrows everything
// computed from these values to 16-bit arithmetic and legalises that with one `v_and_b32 0xffff` per entry -- 6 of a block's 57 VALU
// instructions (k = 5 sums 107.4 -> 105.7 us, k = 6 142.5 -> 140.6; the raw-row tiles' look-ups are better off without:
// `_s6sorh` 211.6 -> 219.2 us with it, the waits move up to the loads)
TPS_DEV uint32_t lut16_at_wide(const uint32_t* lut, uint32_t v2, uint32_t amask1) {
    uint32_t h = lut16_at(lut, v2, amask1);
    asm("" : "+v"(h));
    return h;
}
#endif

// 16-bit candidate sums kept off-chip: explicit global address space (a generic pointer would become FLAT
// instructions, which also count on the LDS counter)
#ifdef TPS_EMU
TPS_DEV void g8_store(uint64_t base, uint32_t i, uint32_t v) { ((uint8_t*)(uintptr_t)base)[i] = (uint8_t)v; }
TPS_DEV void g16_store(uint64_t base, uint32_t i, uint32_t v) { ((uint16_t*)(uintptr_t)base)[i] = (uint16_t)v; }
TPS_DEV uint32_t g16_load(uint64_t base, uint32_t i) { return ((const uint16_t*)(uintptr_t)base)[i]; }
TPS_DEV void g32_store(uint64_t base, uint32_t i, uint32_t v) { ((uint32_t*)(uintptr_t)base)[i] = v; }
TPS_DEV uint32_t g32_load(uint64_t base, uint32_t i) { return ((const uint32_t*)(uintptr_t)base)[i]; }
TPS_DEV uint32_t g32_load_at(uint64_t base, uint32_t byte_off) { return *(const uint32_t*)(uintptr_t)(base + byte_off); }
#else
TPS_DEV void g8_store(uint64_t base, uint32_t i, uint32_t v) {
    typedef __attribute__((address_space(1))) uint8_t* gp_t;
    ((gp_t)(uintptr_t)base)[i] = (uint8_t)v;
}
TPS_DEV void g16_store(uint64_t base, uint32_t i, uint32_t v) {
    typedef __attribute__((address_space(1))) uint16_t* gp_t;
    ((gp_t)(uintptr_t)base)[i] = (uint16_t)v;
}
TPS_DEV uint32_t g16_load(uint64_t base, uint32_t i) {
    typedef const __attribute__((address_space(1))) uint16_t* gp_t;
    return ((gp_t)(uintptr_t)base)[i];
}
// ... at an unsigned 32-bit BYTE offset from a wave-uniform base: one scalar-base load, no 64-bit address arithmetic per lane
TPS_DEV uint32_t g32_load_at(uint64_t base, uint32_t byte_off) {
    typedef const __attribute__((address_space(1))) uint8_t* gb_t;
    typedef const __attribute__((address_space(1))) uint32_t* gp_t;
    return *(gp_t)((gb_t)(uintptr_t)base + byte_off);
}
TPS_DEV void g32_store(uint64_t base, uint32_t i, uint32_t v) {
    typedef __attribute__((address_space(1))) uint32_t* gp_t;
    ((gp_t)(uintptr_t)base)[i] = v;
}
TPS_DEV uint32_t g32_load(uint64_t base, uint32_t i) {
    typedef const __attribute__((address_space(1))) uint32_t* gp_t;
    return ((gp_t)(uintptr_t)base)[i];
}
#endif

// high half of a 32 x 32-bit product (v_mul_hi_u32, full rate) and the sum of the four bytes of a word (v_sad_u8)
TPS_DEV uint32_t mulhi32(uint32_t x, uint32_t y) { return (uint32_t)(((uint64_t)x * (uint64_t)y) >> 32); }
TPS_DEV uint32_t mul24(uint32_t x, uint32_t y) { return (x & 0xFFFFFFu) * (y & 0xFFFFFFu); }      // (the masks let the compiler pick v_mul_u32_u24)
#ifdef TPS_EMU
TPS_DEV uint32_t add_bytes(uint32_t v, uint32_t acc) { return acc + (v & 255u) + ((v >> 8) & 255u) + ((v >> 16) & 255u) + (v >> 24); }
#else
TPS_DEV uint32_t add_bytes(uint32_t v, uint32_t acc) { return __builtin_amdgcn_sad_u8(v, 0u, acc); }
#endif

// a full adder over 32 independent bit positions: the sum bit a ^ b ^ c and the carry (the majority of the three), one
// v_bitop3_b32 each (written out in C++ the compiler shares a ^ b between the two and ends with five instructions)
#ifdef TPS_EMU
TPS_DEV uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
TPS_DEV uint32_t maj3(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (c & (a | b)); }
TPS_DEV uint32_t or_and(uint32_t a, uint32_t b, uint32_t c) { return (a | b) & c; }
#else
TPS_DEV uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
TPS_DEV uint32_t maj3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }
// (a | b) & c, one v_bitop3_b32 as well (the compiler leaves v_or + v_and where c is a literal)
TPS_DEV uint32_t or_and(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xA8); }
#endif

// two 16-bit lanes in one word (lane 0 = bits 0 .. 15): lane-wise a - b; a + the low half of b in both
#ifdef TPS_EMU
TPS_DEV uint32_t pk_u16_sub(uint32_t a, uint32_t b) { return ((a - b) & 0xFFFFu) | (((a >> 16) - (b >> 16)) << 16); }
TPS_DEV uint32_t pk_u16_add(uint32_t a, uint32_t b) { return ((a + b) & 0xFFFFu) | (((a >> 16) + b) << 16); }
#else
typedef unsigned short tps_u16x2 __attribute__((ext_vector_type(2)));
TPS_DEV tps_u16x2 as_u16x2(uint32_t v) { return __builtin_bit_cast(tps_u16x2, v); }
TPS_DEV uint32_t pk_u16_sub(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, as_u16x2(a) - as_u16x2(b)); }                                          // v_pk_sub_u16
TPS_DEV uint32_t pk_u16_add(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, as_u16x2(a) + (tps_u16x2)((unsigned short)b)); }                     // v_pk_add_u16 op_sel_hi:[1,0]
#endif

// 16-byte LDS accesses (p is 16-byte aligned: ds_read_b128 / ds_write_b128)
#ifdef TPS_EMU
TPS_DEV u32x4 lds_load16(const uint32_t* p) { u32x4 v; v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3]; return v; }
TPS_DEV void lds_store16(uint32_t* p, const u32x4& v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
TPS_DEV void lds_store8(uint32_t* p, const u32x2& v) { p[0] = v.x; p[1] = v.y; }
#else
TPS_DEV u32x4 lds_load16(const uint32_t* p) { return *(const u32x4*)p; }
TPS_DEV void lds_store16(uint32_t* p, const u32x4& v) { *(u32x4*)p = v; }
TPS_DEV void lds_store8(uint32_t* p, const u32x2& v) { *(u32x2*)p = v; }
#endif
// 16-bit LDS entries (ds_write_b16 of the low half / ds_read_u16, zero-extended): the resident candidate sums of the default kernels.
// No hardware bound stands behind these: the caller keeps i inside the region.
TPS_DEV void lds16_store(uint16_t* base, uint32_t i, uint32_t v) { base[i] = (uint16_t)v; }
TPS_DEV uint32_t lds16_load(const uint16_t* base, uint32_t i) { return base[i]; }

// Cache policy of the kernels' big output streams (S_w, raw rows: buffer stores): 2 = nt, non-temporal (gfx940+), 0 = default.
// Nothing on the device reads these bytes again (the exact change-point tournament aside); streamed past the caches they cost
// less HBM time: 10 000 x 25 kb reads with raw rows 192.7 -> 176.8 us per launch, config 2 57.4 -> 56.3 us (same box, A/B).
constexpr int STORE_AUX = 2;
// the lane's 8 window sums -> tile_out[8 lane .. 8 lane + 7] as 16-bit values, windows at or past nw_tile dropped
// (g_store_sw8p: the same from the 4 words of 16-bit pairs, window 2 i in the low half of word i)
#ifdef TPS_EMU
TPS_DEV void g_store_sw8(uint16_t* tile_out, int lane, int nw_tile, const uint32_t* v) {
    for (int i = 0; i < 8; ++i)
        if (8 * lane + i < nw_tile) tile_out[8 * lane + i] = (uint16_t)v[i];
}
TPS_DEV void g_store_sw8p(uint16_t* tile_out, int lane, int nw_tile, const uint32_t* p) {
    for (int i = 0; i < 8; ++i)
        if (8 * lane + i < nw_tile) tile_out[8 * lane + i] = (uint16_t)(p[i >> 1] >> (16 * (i & 1)));
}
#else
TPS_DEV void g_store_sw8(uint16_t* tile_out, int lane, int nw_tile, const uint32_t* v) {
    // One buffer_store_dwordx4 (16 contiguous bytes per lane) through a raw buffer descriptor that ends behind the tile's last
    // window: the hardware range-checks every dword of a multi-dword store on its own and drops the ones past the end (GCN3 /
    // Vega ISA, "range checking": raw buffers, store_dword_x{2,3,4} per component) -- the lane that holds the tile's last windows
    // needs no exec masking and no scalar fallback.  A dword is two windows: tiles start at even windows (plan_geometry keeps
    // the windows per tile even, a read's region starts at a multiple of 8), and the odd last window of a read takes the padding
    // slot behind it along.  The descriptor is wave-uniform (SGPRs only).
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)tile_out, 0, ((nw_tile + 1) & ~1) * 2, 0x00020000);
    v4u t;
    t.x = v[0] | (v[1] << 16); t.y = v[2] | (v[3] << 16); t.z = v[4] | (v[5] << 16); t.w = v[6] | (v[7] << 16);      // (v_lshl_or_b32; every S_w < 2^16)
    __builtin_amdgcn_raw_buffer_store_b128(t, rs, lane * 16, 0, STORE_AUX);
}
TPS_DEV void g_store_sw8p(uint16_t* tile_out, int lane, int nw_tile, const uint32_t* p) {
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)tile_out, 0, ((nw_tile + 1) & ~1) * 2, 0x00020000);
    v4u t;
    t.x = p[0]; t.y = p[1]; t.z = p[2]; t.w = p[3];
    __builtin_amdgcn_raw_buffer_store_b128(t, rs, lane * 16, 0, STORE_AUX);
}
#endif
// 16 bytes -> base[cdw .. cdw + 3] (dwords), the dwords at or past n_dw dropped: one range-checked buffer_store_dwordx4 at a
// dword-aligned address instead of four dword stores and a tail case
#ifdef TPS_EMU
TPS_DEV void g_store16_clamped(uint32_t* base, int n_dw, int cdw, const u32x4& t) {
    const uint32_t v[4] = {t.x, t.y, t.z, t.w};
    for (int i = 0; i < 4; ++i)
        if (cdw + i < n_dw) base[cdw + i] = v[i];
}
#else
TPS_DEV void g_store16_clamped(uint32_t* base, int n_dw, int cdw, const u32x4& t) {
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, n_dw * 4, 0x00020000);
    v4u x;
    x.x = t.x; x.y = t.y; x.z = t.z; x.w = t.w;
    __builtin_amdgcn_raw_buffer_store_b128(x, rs, cdw * 4, 0, STORE_AUX);
}
#endif
// v -> base[i] (dwords), dropped where i >= n: one range-checked buffer_store_dword through a wave-uniform descriptor over the n
// dwords -- the bound costs no compare and no exec mask, and an index the caller sets to n (or beyond) is how a lane opts out.
// Default cache policy: the wave reads these values back soon.
#ifdef TPS_EMU
TPS_DEV void g32_store_clamped(uint64_t base, uint32_t n, uint32_t i, uint32_t v) {
    if (i < n) ((uint32_t*)(uintptr_t)base)[i] = v;
}
#else
TPS_DEV void g32_store_clamped(uint64_t base, uint32_t n, uint32_t i, uint32_t v) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)base, 0, (int)(n * 4u), 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b32(v, rs, (int)(i * 4u), 0, 0);
}
#endif

}  // namespace tps
