// topsicle_hip.hip -- libtopsicle_hip.so: kernels + C ABI (include/topsicle_hip.h).
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC  (see __graft_entry__.build()).
// gfx950 only; there is no CPU fallback in this library.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <sys/uio.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "tps_device.h"
#include "tps_motif.h"
#include "tps_variant.h"
#include "tps_tract.h"
#include "tps_ends.h"
#include "tps_anchor.h"
#include "tps_place.h"
#include "tps_align.h"
#include "tps_adapter.h"
#include "tps_refine.h"
#include "tps_methyl.h"
#include "tps_layout.h"
#include "tps_pack.h"
#include "tps_plan.h"
#include "tps_wide.h"
#include "tps_wide_plan.h"

// ======================================================================== kernels
// The scan kernels live in tps_kernels.h (one macro body, instantiated per slide / table kind / outputs).  Compiled alone,
// this file holds all of them; in the split build (-DTPS_KGROUP=0) only the plain and pair kernels, the others come
// from tps_kernels.hip objects.
#include "tps_kernels.h"

extern "C" __global__ void __launch_bounds__(tps::NT * tps::WPG) tps_binseg_kernel(tps::BinsegArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[tps::WPG * tps::BINSEG_SMEM_DW];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * tps::WPG + wave;
    if (r >= a.n_reads) return;
    tps::binseg_read(a, r, smem + wave * tps::BINSEG_SMEM_DW);
}

// every m-th window of a base-slide scan, and the change point of the compacted series (tps_plan.h: stride_base)
extern "C" __global__ void __launch_bounds__(tps::NT * tps::WPG) tps_stride_kernel(tps::StrideArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];      // per wave: the change point's scratch, then the series as 16-bit values
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * tps::WPG + wave;
    if (r >= a.n_reads) return;
    uint32_t* mine = smem + wave * (tps::BINSEG_SMEM_DW + a.s16_dw);
    tps::stride_read(a, r, mine, a.s16_dw ? (uint16_t*)(mine + tps::BINSEG_SMEM_DW) : nullptr);
}

// Wide pattern tables (tps_set_patterns_wide; csrc/tps_wide.h): one wave per read like the scan kernels above, the workgroup's table
// image (hash table, group multiplicities, pattern -> group) copied into LDS once.  Compiled for four waves per SIMD (<= 128 VGPRs).
#if !defined(TPS_KGROUP) || TPS_KGROUP == 0
extern "C" __global__ void __launch_bounds__(tps::NT * tps::WPG, 4) tps_scan_kernel_wide(tps::WideArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    for (int c = 4 * (int)threadIdx.x; c < tps::WIDE_IMG_DW; c += 4 * tps::NT * tps::WPG)
        *(uint4*)(lds + c) = *(const uint4*)(a.img + c);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t* slice = lds + tps::WIDE_IMG_DW + wave * tps::wide_lds_dwords(a);
    const int64_t slot = (int64_t)blockIdx.x * tps::WPG + wave;
    if (slot < a.n_reads) {
        const int64_t r = a.order ? (int64_t)__builtin_amdgcn_readfirstlane(a.order[slot]) : slot;
        tps::wide_read(a, r, slice, lds);
    }
}
#endif

extern "C" __global__ void __launch_bounds__(tps::NT * tps::WPG) tps_followers_kernel(tps::FollowArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[tps::WPG * tps::FOLLOW_LDS_DW];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * tps::WPG + wave;
    if (r >= a.n_reads) return;
    tps::followers_read(a, r, smem + wave * tps::FOLLOW_LDS_DW);
}

// ... on a wide table (tps_set_patterns_wide; followers_wide_read in csrc/tps_wide.h): the workgroup's copy of the table image first,
// as in tps_scan_kernel_wide, then one wave per read
extern "C" __global__ void __launch_bounds__(tps::NT * tps::WPG) tps_followers_kernel_wide(tps::FollowWideArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[tps::WIDE_IMG_DW + tps::WPG * tps::FOLLOWW_LDS_DW];
    for (int c = 4 * (int)threadIdx.x; c < tps::WIDE_IMG_DW; c += 4 * tps::NT * tps::WPG)
        *(uint4*)(smem + c) = *(const uint4*)(a.img + c);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * tps::WPG + wave;
    if (r >= a.n_reads) return;
    tps::followers_wide_read(a, r, smem + tps::WIDE_IMG_DW + wave * tps::FOLLOWW_LDS_DW, smem);
}
static_assert(tps::WIDE_IMG_DW % 4 == 0 && tps::FOLLOWW_LDS_DW % 4 == 0, "16-byte LDS accesses");

// The motif census (tps_batch_motif_census; motif_read in csrc/tps_motif.h): no table, one wave per read.  (Inside the namespace:
// the library exports tps_* names for the C ABI and the scan kernels' stubs only.)
namespace tps {
__global__ void __launch_bounds__(NT * WPG) motif_census_kernel(MotifArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[WPG * MOTIF_LDS_DW];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * WPG + wave;
    if (r >= a.n_reads) return;
    motif_read(a, r, smem + wave * MOTIF_LDS_DW);
}
// The variant census (tps_batch_variant_census; variant_read in csrc/tps_variant.h): no table, one wave per read, the workgroup
// picks the partial profile.
__global__ void __launch_bounds__(NT * WPG) variant_census_kernel(VariantArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[WPG * VARIANT_LDS_DW];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * WPG + wave;
    if (r >= a.n_reads) return;
    variant_read(a, r, smem + wave * VARIANT_LDS_DW, (int)(blockIdx.x % VARIANT_PARTS));
}
// The tract map (tps_batch_tract_map; tract_read in csrc/tps_tract.h): the workgroup copies the call's hit table into LDS once, then
// one wave per read.  Every wave takes part in the copy and the barrier before the waves behind the batch leave.
__global__ void __launch_bounds__(NT * TRACT_WPG) tract_map_kernel(TractArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[TRACT_TABLE_DW + TRACT_WPG * TRACT_LDS_DW];
    const int tab_dw = tract_table_dw(a.w);
    for (int i = (int)threadIdx.x; i < tab_dw; i += NT * TRACT_WPG) smem[i] = a.table[i];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * TRACT_WPG + wave;
    if (r >= a.n_reads) return;
    tract_read(a, r, smem + TRACT_TABLE_DW + wave * TRACT_LDS_DW, smem);
}
// The end sketch (tps_batch_end_sketch; end_sketch_read in csrc/tps_ends.h): the tract map's hit table in LDS, shared by the
// workgroup's waves as there, then one wave per read.
__global__ void __launch_bounds__(NT * ENDS_WPG) end_sketch_kernel(EndSketchArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[TRACT_TABLE_DW + ENDS_WPG * ENDS_LDS_DW];
    const int tab_dw = tract_table_dw(a.w);
    for (int i = (int)threadIdx.x; i < tab_dw; i += NT * ENDS_WPG) smem[i] = a.table[i];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * ENDS_WPG + wave;
    if (r >= a.n_reads) return;
    end_sketch_read(a, r, smem + TRACT_TABLE_DW + wave * ENDS_LDS_DW, smem);
}
// The links between sketches (tps_sketch_links; sketch_links_row in csrc/tps_ends.h): one wave per row.
__global__ void __launch_bounds__(NT * LINKS_WPG) sketch_links_kernel(LinkArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[LINKS_WPG * LINKS_LDS_DW];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i = (int64_t)blockIdx.x * LINKS_WPG + wave;
    if (i >= a.n) return;
    sketch_links_row(a, i, smem + wave * LINKS_LDS_DW);
}
// The kept windows (tps_batch_end_window; end_window_read in csrc/tps_anchor.h): the sketch's layout -- the hit table shared by the
// workgroup's waves, one wave per read.
__global__ void __launch_bounds__(NT * ENDS_WPG) end_window_kernel(EndWindowArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[TRACT_TABLE_DW + ENDS_WPG * ENDS_LDS_DW];
    const int tab_dw = tract_table_dw(a.w);
    for (int i = (int)threadIdx.x; i < tab_dw; i += NT * ENDS_WPG) smem[i] = a.table[i];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * ENDS_WPG + wave;
    if (r >= a.n_reads) return;
    end_window_read(a, r, smem + TRACT_TABLE_DW + wave * ENDS_LDS_DW, smem);
}
// The offsets between windows (tps_window_offsets; window_offsets_row in csrc/tps_anchor.h): one wave per query row.
__global__ void __launch_bounds__(NT * OFFSETS_WPG) window_offsets_kernel(OffsetArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[OFFSETS_WPG * OFFSETS_LDS_DW];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i = (int64_t)blockIdx.x * OFFSETS_WPG + wave;
    if (i >= a.n) return;
    window_offsets_row(a, i, smem + wave * OFFSETS_LDS_DW);
}
// The windows placed on a reference's (tps_window_place; window_place_row in csrc/tps_place.h): one wave per query row.
__global__ void __launch_bounds__(NT * PLACE_WPG) window_place_kernel(PlaceArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[PLACE_WPG * PLACE_LDS_DW];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i = (int64_t)blockIdx.x * PLACE_WPG + wave;
    if (i >= a.n) return;
    window_place_row(a, i, smem + wave * PLACE_LDS_DW);
}
// One window aligned against another base by base (tps_window_align; window_align_row in csrc/tps_align.h): one wave per pair.  The
// LDS is dynamic: the call sizes every wave's slice by its span and its longest query.
__global__ void __launch_bounds__(NT * ALIGN_WPG) window_align_kernel(AlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i = (int64_t)blockIdx.x * ALIGN_WPG + wave;
    if (i >= a.n) return;
    window_align_row(a, i, smem + wave * align_lds_dw(a.span, a.cdw, a.rows));
}
// The adapters at the telomere end (tps_batch_adapter_find; adapter_read in csrc/tps_adapter.h): no table, one wave per read, one lane
// per pattern.
__global__ void __launch_bounds__(NT * ADAPTER_WPG) adapter_find_kernel(AdapterArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[ADAPTER_WPG * ADAPTER_LDS_DW];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * ADAPTER_WPG + wave;
    if (r >= a.n_reads) return;
    adapter_read(a, r, smem + wave * ADAPTER_LDS_DW);
}
// The boundary at base resolution (tps_batch_boundary_refine; refine_read in csrc/tps_refine.h): the tract map's hit table in LDS,
// shared by the workgroup's waves as there, then one wave per read.  The LDS is dynamic: the call sizes every wave's slice by the
// longest region of the batch.
__global__ void __launch_bounds__(NT * REFINE_WPG) boundary_refine_kernel(RefineArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int tab_dw = tract_table_dw(a.w);
    for (int i = (int)threadIdx.x; i < tab_dw; i += NT * REFINE_WPG) smem[i] = a.table[i];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * REFINE_WPG + wave;
    if (r >= a.n_reads) return;
    refine_read(a, r, smem + TRACT_TABLE_DW + wave * refine_lds_dw(a.bal_dw), smem);
}
// Base modifications against the boundary (tps_batch_mod_profile; mod_read in csrc/tps_methyl.h): no table, one wave per read.
__global__ void __launch_bounds__(NT * MOD_WPG) mod_profile_kernel(ModArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t smem[MOD_WPG * MOD_LDS_DW];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * MOD_WPG + wave;
    if (r >= a.n_reads) return;
    mod_read(a, r, smem + wave * MOD_LDS_DW);
}
}  // namespace tps

// ASCII -> packed batch (tps_pack.h), one workgroup per read, one thread per word of 16 bases.  Runs once per
// tps_batch_upload, right behind the copy of the ASCII bytes; the scan kernels only ever see the packed batch.
// bits 1-2 of an ASCII letter: A,C,T,G (either case) -> 0,1,2,3; one v_dot4_u32_u8 packs 4 bases; a v_perm rebuilds the
// lower-case letter each code stands for and any byte that differs from it in more than the case bit is invalid.
extern "C" __global__ void __launch_bounds__(256) tps_pack_kernel(const uint8_t* bases, const int64_t* offsets, tps_read_desc* desc,
                                                                   uint32_t* seq2, uint16_t* inv, int64_t n_reads, uint32_t* any_flag) {
    const int64_t r = blockIdx.x;
    if (r >= n_reads) return;
    const int64_t off = offsets[r];
    const int64_t L = desc[r].len;
    const int64_t w0 = desc[r].word_off;
    const int64_t nw = ((L + 63) / 64) * 4;
    uint32_t any = 0;
    for (int64_t w = threadIdx.x; w < nw; w += 256) {
        const int64_t left = L - 16 * w;               // bases of this word (<= 0: padding up to the quad boundary)
        uint32_t packed = 0, bad = 0;
        if (left > 0) {
            // the read starts at an arbitrary byte: five aligned dwords + byte funnel shifts
            const uintptr_t p = (uintptr_t)(bases + off + 16 * w);
            const uint32_t* q = (const uint32_t*)(p & ~(uintptr_t)3);
            const uint32_t sh = (uint32_t)(p & 3u);
            const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3], d4 = q[4];
            uint32_t v[4] = {__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                             __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh)};
            uint32_t any_bad = 0, b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t y = v[i] & 0x06060606u;
                packed |= (tps::udot4(y, 0x40100401u) >> 1) << (8 * i);
                b[i] = (v[i] ^ tps::perm(0x00670074u, 0x00630061u, y)) & 0xDFDFDFDFu;
                any_bad |= b[i];
            }
            if (any_bad) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((b[i] >> (8 * j)) & 255u) bad |= 1u << (4 * i + j);
            }
            if (left < 16) {
                packed &= (1u << (2 * (int)left)) - 1u;
                bad &= (1u << (int)left) - 1u;
            }
        }
        seq2[w0 + w] = packed;
        inv[w0 + w] = (uint16_t)bad;
        any |= bad;
    }
    if (any) {
        atomicOr(&desc[r].flags, TPS_RD_HAS_INVALID);
        *any_flag = 1u;                            // (mapped host word: the batch has a read with a non-ACGT letter)
    }
}

// BAM's 4-bit base codes -> packed batch (tps_batch_upload_nib4), one workgroup per read, one thread per word of 16 bases.  A word's
// 16 codes are one 64-bit load (two for a reverse-strand read, whose window starts at any code: a funnel shift), the two codes of each
// byte swapped so that code t sits in nibble t; v_bfrev of the 64 bits then reverses the order of the codes AND complements each of
// them (on these codes the IUPAC complement is the bit reversal of the code: A = 1 <-> T = 8, C = 2 <-> G = 4, ...).  Code c becomes
// the 2-bit code of its letter's ASCII ((ASCII >> 1) & 3: "=ACMGRSVTWYHKDBN" -> NIB4_CODE2) and is flagged in inv unless it is one of
// A, C, G, T: bit-identical to tps_pack_kernel on the records' ASCII text.  A read's codes take whole 16-byte units of the nibble
// buffer from a 16-byte boundary on (the host checks it), so a 64-bit load that holds one of its codes never leaves them.
constexpr uint32_t NIB4_CODE2 = 0xd90ed792u;         // bits [2c, 2c+1]: the code of BAM letter c
constexpr uint32_t NIB4_ACGT = 0x0116u;              // bit c: code c is one of A (1), C (2), G (4), T (8)
__device__ __forceinline__ uint64_t nib_swap(uint64_t v) { return ((v >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((v & 0x0F0F0F0F0F0F0F0Full) << 4); }
extern "C" __global__ void __launch_bounds__(256) tps_pack_kernel_nib4(const uint8_t* nib, const tps_nib_src* src, const tps_read_desc* desc,
                                                                        uint32_t* seq2, uint16_t* inv, int64_t n_reads) {
    const int64_t r = blockIdx.x;
    if (r >= n_reads) return;
    const int64_t L = desc[r].len;
    const int64_t w0 = desc[r].word_off;
    const int64_t nw = ((L + 63) / 64) * 4;
    const uint64_t* q = (const uint64_t*)(nib + src[r].off);
    const bool rev = (src[r].flags & TPS_NIB_REVERSE) != 0u;
    for (int64_t w = threadIdx.x; w < nw; w += 256) {
        const int64_t left = L - 16 * w;               // bases of this word (<= 0: padding up to the quad boundary)
        uint32_t packed = 0, bad = 0;
        if (left > 0) {
            uint64_t x;
            if (!rev) {
                x = nib_swap(q[w]);
            } else {
                // output bases 16 w .. 16 w + 15 are the complements of stored codes L - 1 - 16 w down to a = L - 16 - 16 w (a < 0 only
                // in the read's last word, where the codes below 0 land on output bases >= L and are masked off)
                const int64_t a = L - 16 - 16 * w;
                const int64_t qa = a >> 4;                                       // (floor division)
                const uint32_t sh = (uint32_t)(a & 15) * 4u;
                const uint64_t lo = qa >= 0 ? nib_swap(q[qa]) : 0ull;
                x = sh ? (lo >> sh) | (nib_swap(q[qa + 1]) << (64u - sh)) : lo;
                x = __brevll(x);
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const uint32_t c = (uint32_t)(x >> (4 * t)) & 15u;
                packed |= ((NIB4_CODE2 >> (2 * c)) & 3u) << (2 * t);
                bad |= ((~NIB4_ACGT >> c) & 1u) << t;
            }
            if (left < 16) {
                packed &= (1u << (2 * (int)left)) - 1u;
                bad &= (1u << (int)left) - 1u;
            }
        }
        seq2[w0 + w] = packed;
        inv[w0 + w] = (uint16_t)bad;
    }
}

// ======================================================================== host side
namespace {

thread_local std::string g_err;

// Pinned host buffers handed out by tps_host_alloc, process-wide: the pipeline allocates its staging pool through ONE context and
// every context uploads from it (hipHostMallocPortable: pinned for all devices); tps_batch_upload_packed copies asynchronously
// whenever its sources lie in registered buffers, whoever allocated them.
std::mutex g_pinned_mu;
std::map<uintptr_t, size_t> g_pinned;            // base -> bytes
bool is_pinned(const void* p, size_t bytes) {
    if (!p || !bytes) return true;
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    auto it = g_pinned.upper_bound((uintptr_t)p);
    if (it == g_pinned.begin()) return false;
    --it;
    return (uintptr_t)p + bytes <= it->first + it->second;
}

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail(TPS_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

constexpr int64_t PAD = 64;          // readable bytes before / after the concatenated bases
constexpr int INTERNAL_SLOT = TPS_MAX_SLOTS;

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool borrowed = false;               // p belongs to another context's slot (tps_batch_share): never freed, never grown here
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;      // (owns p: whatever holds a DevBuf frees it by going away, tps_ctx_destroy names none of them)
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t bytes) {
        if (borrowed) { p = nullptr; cap = 0; borrowed = false; }
        if (bytes <= cap) return TPS_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return TPS_OK;
    }
    void release() { if (p && !borrowed) (void)hipFree(p); p = nullptr; cap = 0; borrowed = false; }
    void borrow(const DevBuf& o) { release(); p = o.p; cap = o.cap; borrowed = true; }
};

struct Slot {
    DevBuf seq2, inv, desc, tails, results, c_start, c_end, win_off, win_off16, sums, raw, stamps, lc, order;
    int64_t n_words = 0;                 // words of seq2 / inv in use
    bool inv_valid = true;               // false: the batch came packed without an inv array (no read is flagged)
    bool any_invalid = true;             // some read of the batch is flagged TPS_RD_HAS_INVALID (the kernels then stage the invalid masks)
    std::vector<int64_t> h_offsets;      // host copy of offsets (n+1)
    tps::BatchLayout lay;                // window layout and dispatch order of the last plan (tps::plan_batch_layout)
    std::vector<uint16_t> h_sums16;      // download scratch
    tps_read_result* h_results = nullptr;   // pinned
    size_t h_results_cap = 0;
    int64_t n = -1;
    bool has_tails = false;
    // cached plan
    bool planned = false;
    tps_params plan_prm{};
    int plan_k = 0, plan_p = 0;
    uint32_t plan_dup = 0, plan_so = 0;   // the plan depends on whether the pattern list holds duplicate / self-overlapping k-mers
    tps::ScanArgs args{};
    size_t lds_bytes = 0;
    const char* kernel_name = "";       // what the last scan of this slot launched
    bool scanned = false;
    uint32_t last_flags = 0;
    // scans at a multiple of a fused kernel's slide (tps::stride_base): the base-slide scan runs in a slot of its own that borrows this
    // slot's batch; `sub_stale` = the batch has changed since it was borrowed
    Slot* sub = nullptr;
    bool sub_stale = true;
    // (a base-slide slot) where the scan may store every 2nd raw row itself: the requesting scan's buffer and window layout
    void* ext_raw = nullptr;
    const int64_t* ext_raw_win_off = nullptr;
    bool rows_inline = false;            // ... and it did (last scan)
    int stride_base = 0;                 // of the cached plan: 0 = the planned kernel runs itself
    std::string info_name;               // kernel_name of a strided scan ("<base kernel> every <m>th window")
    // cached plan of the wide kernel (do_scan_wide): by parameters and by the table's serial number -- any tps_set_patterns* call
    // drops it, like `planned`
    bool wplanned = false;
    tps_params wplan_prm{};
    uint64_t wplan_table = 0;
    tps::WideArgs wargs{};
    ~Slot() {
        if (h_results) (void)hipHostFree(h_results);
        delete sub;
    }
};

// The scan kernels of tps_kernels.h by family (table kind and outputs) and slide; {} = no such instantiation.  TPS_K: the name
// tps_batch_kernel_info reports is the symbol.
struct ScanKernel { const void* fn; const char* name; };
#define TPS_K(sym) {(const void*)sym, #sym}
enum ScanFamily { KF_PLAIN, KF_PAIR, KF_PAIRQ, KF_RAW, KF_SO, KF_SOL, KF_SOR, KF_SORH, KF_COUNT };
constexpr int KSLIDE_MIN = 3, KSLIDE_MAX = 12;
const ScanKernel GENERIC_KERNEL = TPS_K(tps_scan_kernel);
const ScanKernel FUSED_KERNELS[KF_COUNT][KSLIDE_MAX - KSLIDE_MIN + 1] = {
    // plain and pair table (sums only, no self-overlap): the default kernels have every slide a window of 100 allows
    {TPS_K(tps_scan_kernel_s3), TPS_K(tps_scan_kernel_s4), TPS_K(tps_scan_kernel_s5), TPS_K(tps_scan_kernel_s6), TPS_K(tps_scan_kernel_s7),
     TPS_K(tps_scan_kernel_s8), TPS_K(tps_scan_kernel_s9), TPS_K(tps_scan_kernel_s10), TPS_K(tps_scan_kernel_s11), TPS_K(tps_scan_kernel_s12)},
    {TPS_K(tps_scan_kernel_s3p), TPS_K(tps_scan_kernel_s4p), TPS_K(tps_scan_kernel_s5p), TPS_K(tps_scan_kernel_s6p), TPS_K(tps_scan_kernel_s7p),
     TPS_K(tps_scan_kernel_s8p), TPS_K(tps_scan_kernel_s9p), TPS_K(tps_scan_kernel_s10p), TPS_K(tps_scan_kernel_s11p), TPS_K(tps_scan_kernel_s12p)},
    // the others keep slides 5 .. 8: 16-bit pair table (k = 5), raw rows, self-overlap sums (periods 5 and 6; 2 .. 4), self-overlap raw
    // rows (32-bit fields; 16-bit field indices)
    {{}, {}, TPS_K(tps_scan_kernel_s5q), TPS_K(tps_scan_kernel_s6q), TPS_K(tps_scan_kernel_s7q), TPS_K(tps_scan_kernel_s8q)},
    {{}, {}, TPS_K(tps_scan_kernel_s5r), TPS_K(tps_scan_kernel_s6r), TPS_K(tps_scan_kernel_s7r), TPS_K(tps_scan_kernel_s8r)},
    {{}, {}, TPS_K(tps_scan_kernel_s5so), TPS_K(tps_scan_kernel_s6so), TPS_K(tps_scan_kernel_s7so), TPS_K(tps_scan_kernel_s8so)},
    {{}, {}, TPS_K(tps_scan_kernel_s5sol), TPS_K(tps_scan_kernel_s6sol), TPS_K(tps_scan_kernel_s7sol), TPS_K(tps_scan_kernel_s8sol)},
    {{}, {}, TPS_K(tps_scan_kernel_s5sor), TPS_K(tps_scan_kernel_s6sor), TPS_K(tps_scan_kernel_s7sor), TPS_K(tps_scan_kernel_s8sor)},
    {{}, {}, TPS_K(tps_scan_kernel_s5sorh), TPS_K(tps_scan_kernel_s6sorh), TPS_K(tps_scan_kernel_s7sorh), TPS_K(tps_scan_kernel_s8sorh)},
};
#undef TPS_K

struct EventPair { hipEvent_t a, b; };

}  // namespace

struct tps_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipDeviceProp_t prop{};
    // dev: [4^k masks][pair table, k <= 4][ready-made LDS images of the table for the fused kernels, each a multiple of 4 dwords:
    // mask << 16 | count, one-hot fields, 16-bit masks -- a workgroup copies its image in 16-byte pieces instead of converting it]
    struct Table { DevBuf dev; int P = 0, k = 0; std::string key; tps::PatInfo pat{}; size_t off_e32 = 0, off_fld = 0, off_m16 = 0, off_f16 = 0, off_p16 = 0, off_pfld = 0; };
    std::deque<Table> tables;         // resident pattern tables (deque: pointers to elements stay valid)
    Table* lut_cur = nullptr;
    // wide tables (tps_set_patterns_wide): the image tps_scan_kernel_wide copies into LDS; `serial` names a table in the slots' plans
    struct WideTable { DevBuf dev; std::string key; int P = 0, k = 0; tps::WidePat pat{}; uint64_t serial = 0; };
    std::deque<WideTable> wtables;
    WideTable* wide_cur = nullptr;    // non-null: the current table is a wide one, tps_batch_scan launches the wide kernel
    size_t wtable_rr = 0;
    uint64_t table_serial = 0;
    size_t lds_set_wide = 0;
    size_t table_rr = 0;
    DevBuf follow_picks, follow_hist; // outputs of tps_batch_kmer_followers
    DevBuf motif_hits, motif_counts;  // outputs of tps_batch_motif_census
    DevBuf variant_in, variant_counts, variant_prof;      // tps_batch_variant_census: tails / begin / end, its outputs
    std::vector<unsigned long long> h_variant_prof;        // ... the partial profiles as downloaded
    DevBuf tract_table, tract_out;    // tps_batch_tract_map: the call's hit table; tracts, found and totals behind one another
    DevBuf ends_in, ends_out;         // tps_batch_end_sketch: tails / begin / end; sketch and kept behind one another (its table is tract_table)
    DevBuf links_t, links_out;        // tps_sketch_links: the sketches bucket-major; degree, links and matches behind one another
    DevBuf window_out;                // tps_batch_end_window: codes and keep behind one another (its inputs are ends_in, its table tract_table)
    DevBuf offsets_in, offsets_out;   // tps_window_offsets: codes, keep, length and ref; offset, votes and second behind one another
    DevBuf place_in, place_idx, place_out;   // tps_window_place: the queries' codes, keep and length; the index's dir, keys and ent; the seven outputs behind one another
    DevBuf align_in, align_out, align_pile;   // tps_window_align: both sets' codes and lengths, ref, centre and pile_row; stat and cols behind one another; the pile
    DevBuf adapter_in, adapter_out;   // tps_batch_adapter_find: Peq, lengths, tails / begin / end; the hits
    DevBuf mod_in, mod_out;           // tps_batch_mod_profile: tails / begin / end / origin, mod_off, delta, prob; the rows and the bins behind them
    DevBuf refine_in, refine_out;     // tps_batch_boundary_refine: tails / begin / end / at; the rows (its table is tract_table)
    DevBuf ascii, ascii_off;          // staging of tps_batch_upload: ASCII bases + offsets, packed on the device right after the copy
    DevBuf nib, nib_src;              // staging of tps_batch_upload_nib4: BAM base codes + where each read's are, expanded right after the copy
    std::set<void*> pinned;           // host buffers handed out by tps_host_alloc
    std::vector<tps_read_desc> h_desc;   // scratch of the ASCII upload path
    tps::PatInfo pat{};
    bool have_pat = false;
    Slot slots[TPS_MAX_SLOTS + 1];
    std::vector<EventPair> ev_pool;
    size_t ev_used = 0;      // next free event pair (never rewound: re-recording old events was measured slow)
    size_t ev_base = 0;      // first pair of the current measurement window
    tps::PlanKnobs knobs = tps::product_knobs();     // tps_ctx_debug_option: tests / diagnostics only; the library reads no environment
    int want_stamps = 0;
    int no_events = 0;
    int no_inline_rows = 0;           // tps_ctx_debug_option "no_inline_rows": strided scans at twice the base slide copy their raw rows like the others (A/B of ScanArgs::raw_m)
    int no_stride = 0;                // tps_ctx_debug_option "no_stride": slides that are a multiple of a fused kernel's keep the generic kernel (A/B of tps::stride_base)
    int file_order = 0;               // tps_ctx_debug_option "file_order": wave slot i takes read i whatever the reads' lengths (A/B of tps::plan_dispatch_order)
    int poison = 0;                   // tps_ctx_debug_option "poison": 1..255 = every call fills the output and scratch buffers it is about to use with this byte (tests: a byte nobody writes shows)
    int event_stride = 1;             // time every event_stride-th launch (tps_ctx_debug_option "event_stride"): timing costs ~3.5 us per launch
    uint64_t launch_seq = 0;
    size_t lds_set_refine = 0;       // ... of boundary_refine_kernel
    size_t lds_set_align = 0;        // ... of window_align_kernel
    size_t lds_set_generic = 0;      // hipFuncAttributeMaxDynamicSharedMemorySize as last raised, per scan kernel
    size_t lds_set_fused[KF_COUNT][KSLIDE_MAX - KSLIDE_MIN + 1] = {};
    uint32_t* h_flag = nullptr;      // mapped host word the pack kernel raises when a read has a non-ACGT letter
    hipEvent_t share_ev = nullptr;   // tps_batch_share: orders this context's stream behind the lender's upload
    void* raw_stage[2] = {nullptr, nullptr};    // tps_batch_raw_to_fd: two pinned pieces, one being written while the other is filled
    hipEvent_t raw_ev[2] = {nullptr, nullptr};
};

namespace {

int bind(tps_ctx* c) {
    if (!c) return fail(TPS_E_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    return TPS_OK;
}

using tps::window_count;

// Debug option "poison" (include/topsicle_hip.h): fills a device buffer this call is about to use as output or scratch, over its whole
// capacity, on the context's stream -- ahead of the library's own clearing memsets and of the launch.  A borrowed buffer is another
// context's (or another scan's) to fill, never this one's.  Call sites test c->poison themselves: one not-taken branch when it is off.
int poison_fill(tps_ctx* c, DevBuf& b) {
    if (b.borrowed || !b.p || !b.cap) return TPS_OK;
    HIP_TRY(hipMemsetAsync(b.p, c->poison, b.cap, c->stream));
    return TPS_OK;
}
#define TPS_POISON(buf)                                             \
    do {                                                            \
        if (c->poison && (rc = poison_fill(c, (buf)))) return rc;   \
    } while (0)

// LDS one workgroup may use, in dwords: what the device reports, at most gfx950's 160 KB; 64 KB where it reports nothing
int64_t lds_budget_dw(const tps_ctx* c) {
    return (int64_t)(c->prop.sharedMemPerBlock > 0 ? std::min<size_t>(c->prop.sharedMemPerBlock, 160 * 1024) : 64 * 1024) / 4;
}

int plan_lds(tps_ctx* c, Slot& sl, const tps_params& prm, int64_t max_nwin) {
    sl.args.pat = c->pat;                          // the plan looks at dup_mask
    std::string err = tps::plan_geometry(sl.args, prm, c->pat.k, c->pat.P, max_nwin, lds_budget_dw(c), c->knobs);
    if (!err.empty()) return fail(TPS_E_CAPACITY, "%s", err.c_str());
    sl.lds_bytes = (size_t)tps::wg_lds_dwords(sl.args) * 4;
    return TPS_OK;
}

int check_params(const tps_params& p) {
    if (p.window < 1 || p.slide < 1 || p.trimfirst < 0 || p.maxlen < 0 || p.no_bp < 0)
        return fail(TPS_E_ARG, "bad window/slide/trimfirst/maxlen/no_bp");
    if ((p.flags & TPS_F_BINSEG) && (p.jump < 1 || p.min_size < 1))
        return fail(TPS_E_ARG, "bad jump/min_size");
    if (p.slide > 4096 || p.window > 65536 || p.jump > 4096) return fail(TPS_E_CAPACITY, "window/slide/jump too large");
    if ((p.flags & TPS_F_WINDOWS) && p.jump < 1) return fail(TPS_E_ARG, "jump must be >= 1");
    return TPS_OK;
}

// what every scan checks before it plans, whatever the table
int check_scan(const Slot& sl, const tps_params& prm) {
    int rc;
    if (sl.n < 0) return fail(TPS_E_STATE, "no batch uploaded in this slot");
    if ((rc = check_params(prm))) return rc;
    if (!(prm.flags & TPS_F_STEP1) && (prm.flags & TPS_F_TAILS_IN) && !sl.has_tails)
        return fail(TPS_E_STATE, "TPS_F_TAILS_IN without tps_batch_set_tails");
    return TPS_OK;
}

// a table or knob change: every cached plan goes, the strided scans' hidden sub-slots included
void drop_plans(tps_ctx* c) {
    for (auto& sl : c->slots) {
        sl.planned = false;
        sl.wplanned = false;
        if (sl.sub) { sl.sub->planned = false; sl.sub->wplanned = false; }
    }
}

void reset_slot(Slot& sl, int64_t n, int64_t n_words) {
    sl.sub_stale = true;
    sl.wplanned = false;
    sl.n = n;
    sl.n_words = n_words;
    sl.has_tails = false;
    sl.planned = false;
    sl.scanned = false;
}

int ensure_packed(tps_ctx* c, Slot& sl, int64_t n, int64_t n_words) {
    int rc;
    if ((rc = sl.seq2.ensure((size_t)std::max<int64_t>(n_words, 4) * 4))) return rc;
    if ((rc = sl.inv.ensure((size_t)std::max<int64_t>(n_words, 4) * 2))) return rc;
    if ((rc = sl.desc.ensure((size_t)std::max<int64_t>(n, 1) * sizeof(tps_read_desc)))) return rc;
    TPS_POISON(sl.seq2);          // (ahead of the copies and of the pack / expand kernel that write them)
    TPS_POISON(sl.inv);
    TPS_POISON(sl.desc);
    return TPS_OK;
}

// read i of a batch that comes packed: its descriptor lies inside the n_words words of the batch
int check_desc(const tps_read_desc& d, int64_t i, int64_t n_words) {
    if (d.len < 0 || d.word_off < 0 || (d.word_off & 3) || d.word_off + tps::packed_words(d.len) > n_words)
        return fail(TPS_E_ARG, "read %lld: descriptor outside the packed batch (word_off %lld, len %d, %lld words)", (long long)i,
                    (long long)d.word_off, d.len, (long long)n_words);
    return TPS_OK;
}

// the mapped pinned buffer the kernels write a batch's results into
int ensure_h_results(Slot& sl, int64_t n) {
    if (sl.h_results_cap >= (size_t)n) return TPS_OK;
    if (sl.h_results) (void)hipHostFree(sl.h_results);
    sl.h_results = nullptr;
    sl.h_results_cap = 0;
    size_t want = (size_t)n + (size_t)n / 8 + 16;
    HIP_TRY(hipHostMalloc((void**)&sl.h_results, want * sizeof(tps_read_result), hipHostMallocMapped));
    sl.h_results_cap = want;
    return TPS_OK;
}

// option "poison" for the mapped pinned result array: filled by the host once the stream has drained, so the fill is ordered behind
// whatever the stream still wrote there and ahead of the launch that follows
int poison_h_results(tps_ctx* c, Slot& sl) {
    if (!sl.h_results) return TPS_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    memset(sl.h_results, c->poison, sl.h_results_cap * sizeof(tps_read_result));
    return TPS_OK;
}

// The events of the next scan launch: a pair from the pool if it is timed, {nullptr, nullptr} if not (an inner base-slide scan --
// the strided scan around it is the launch that counts, so it does not advance launch_seq either --, option no_events, or all
// but every event_stride-th launch).  tps_kernel_time_ms adds up the pairs handed out since the last reset.
int next_events(tps_ctx* c, bool inner, EventPair& ev) {
    if (c->ev_used == c->ev_pool.size()) {
        if (c->ev_pool.size() >= 16384) {
            c->ev_used = c->ev_base = 0;                  // wrap: the measurement window restarts
        } else {
            // events are created in batches, never one per launch (hipEventCreate costs ~60 us)
            const size_t grow = c->ev_pool.empty() ? 512 : c->ev_pool.size();
            for (size_t i = 0; i < grow; ++i) {
                EventPair ep;
                HIP_TRY(hipEventCreate(&ep.a));
                HIP_TRY(hipEventCreate(&ep.b));
                c->ev_pool.push_back(ep);
            }
        }
    }
    const bool timed = !inner && !c->no_events && (c->launch_seq++ % (uint64_t)c->event_stride) == 0;
    ev = timed ? c->ev_pool[c->ev_used++] : EventPair{nullptr, nullptr};
    return TPS_OK;
}

// ASCII batch -> HBM -> packed batch (tps_pack_kernel).  The ASCII copy only lives in the context's staging buffer.
int do_upload(tps_ctx* c, Slot& sl, const uint8_t* bases, const int64_t* offsets, int64_t n) {
    if (n < 0 || !offsets || (n > 0 && !bases)) return fail(TPS_E_ARG, "bad batch pointers");
    if (offsets[0] != 0) return fail(TPS_E_ARG, "offsets[0] must be 0");
    for (int64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return fail(TPS_E_ARG, "offsets not monotone at %lld", (long long)i);
        if (offsets[i + 1] - offsets[i] > 0x7FFFFFFFll) return fail(TPS_E_CAPACITY, "read %lld is longer than 2^31 - 1 bases", (long long)i);
    }
    const int64_t total = offsets[n];
    c->h_desc.resize((size_t)std::max<int64_t>(n, 1));
    const int64_t n_words = tps::pack_layout(offsets, n, c->h_desc.data());
    int rc;
    if ((rc = ensure_packed(c, sl, n, n_words))) return rc;
    if ((rc = c->ascii.ensure((size_t)(total + 2 * PAD + 32)))) return rc;
    if ((rc = c->ascii_off.ensure((size_t)(n + 1) * 8))) return rc;
    uint8_t* d = (uint8_t*)c->ascii.p;
    if (total) HIP_TRY(hipMemcpyAsync(d + PAD, bases, (size_t)total, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ascii_off.p, offsets, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n) HIP_TRY(hipMemcpyAsync(sl.desc.p, c->h_desc.data(), (size_t)n * sizeof(tps_read_desc), hipMemcpyHostToDevice, c->stream));
    if (n) {
        if (!c->h_flag) HIP_TRY(hipHostMalloc((void**)&c->h_flag, 64, hipHostMallocMapped));
        *c->h_flag = 0u;
        hipLaunchKernelGGL(tps_pack_kernel, dim3((unsigned)n), dim3(256), 0, c->stream, (const uint8_t*)d + PAD,
                           (const int64_t*)c->ascii_off.p, (tps_read_desc*)sl.desc.p, (uint32_t*)sl.seq2.p, (uint16_t*)sl.inv.p, n, c->h_flag);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(c->stream));       // the caller's buffers and h_desc are free again
    sl.h_offsets.assign(offsets, offsets + n + 1);
    sl.inv_valid = true;
    sl.any_invalid = n > 0 && *(volatile uint32_t*)c->h_flag != 0u;
    reset_slot(sl, n, n_words);
    return TPS_OK;
}

// Host-packed batch: three plain copies.  Pinned sources (tps_host_alloc) are copied asynchronously.
int do_upload_packed(tps_ctx* c, Slot& sl, const uint32_t* seq2, const uint16_t* inv, const tps_read_desc* desc, int64_t n, int64_t n_words) {
    if (n < 0 || n_words < 0 || (n > 0 && !desc) || (n_words > 0 && !seq2)) return fail(TPS_E_ARG, "bad packed batch pointers");
    int rc;
    sl.h_offsets.resize((size_t)n + 1);
    int64_t acc = 0, need = 0;
    bool flagged = false;
    for (int64_t i = 0; i < n; ++i) {
        const tps_read_desc& d = desc[i];
        if ((rc = check_desc(d, i, n_words))) return rc;
        sl.h_offsets[(size_t)i] = acc;
        acc += d.len;
        need = std::max(need, d.word_off + tps::packed_words(d.len));
        flagged = flagged || (d.flags & TPS_RD_HAS_INVALID);
    }
    sl.h_offsets[(size_t)n] = acc;
    if (flagged && !inv) return fail(TPS_E_ARG, "a read is flagged TPS_RD_HAS_INVALID but inv is NULL");
    if ((rc = ensure_packed(c, sl, n, n_words))) return rc;
    if (n_words) HIP_TRY(hipMemcpyAsync(sl.seq2.p, seq2, (size_t)n_words * 4, hipMemcpyHostToDevice, c->stream));
    if (n_words && inv) HIP_TRY(hipMemcpyAsync(sl.inv.p, inv, (size_t)n_words * 2, hipMemcpyHostToDevice, c->stream));
    if (n) HIP_TRY(hipMemcpyAsync(sl.desc.p, desc, (size_t)n * sizeof(tps_read_desc), hipMemcpyHostToDevice, c->stream));
    const bool all_pinned = is_pinned(seq2, (size_t)n_words * 4) && is_pinned(inv, inv ? (size_t)n_words * 2 : 0) && is_pinned(desc, (size_t)n * sizeof(tps_read_desc));
    if (!all_pinned) HIP_TRY(hipStreamSynchronize(c->stream));     // ordinary memory: the copy is over when the call returns
    sl.inv_valid = inv != nullptr;
    sl.any_invalid = flagged;
    reset_slot(sl, n, n_words);
    return TPS_OK;
}

// BAM records: their 4-bit codes, where each read's are and the descriptors go up; tps_pack_kernel_nib4 writes seq2 / inv.  Pinned
// sources (tps_host_alloc) are copied asynchronously.  The descriptors come from the caller with exact TPS_RD_HAS_INVALID flags.
int do_upload_nib4(tps_ctx* c, Slot& sl, const uint8_t* nib, int64_t nib_bytes, const tps_nib_src* src, const tps_read_desc* desc, int64_t n,
                   int64_t n_words) {
    if (n < 0 || n_words < 0 || nib_bytes < 0 || (n > 0 && (!desc || !src)) || (nib_bytes > 0 && !nib)) return fail(TPS_E_ARG, "bad nib4 batch pointers");
    int rc;
    sl.h_offsets.resize((size_t)n + 1);
    int64_t acc = 0;
    bool flagged = false;
    for (int64_t i = 0; i < n; ++i) {
        const tps_read_desc& d = desc[i];
        if ((rc = check_desc(d, i, n_words))) return rc;
        const int64_t units = (((int64_t)d.len + 1) / 2 + 15) & ~(int64_t)15;            // the 16-byte units the kernel may load from
        if (src[i].off < 0 || (src[i].off & 15) || src[i].off + units > nib_bytes)
            return fail(TPS_E_ARG, "read %lld: codes outside the nibble buffer (off %lld, len %d, %lld bytes)", (long long)i,
                        (long long)src[i].off, d.len, (long long)nib_bytes);
        sl.h_offsets[(size_t)i] = acc;
        acc += d.len;
        flagged = flagged || (d.flags & TPS_RD_HAS_INVALID);
    }
    sl.h_offsets[(size_t)n] = acc;
    if ((rc = ensure_packed(c, sl, n, n_words))) return rc;
    if ((rc = c->nib.ensure((size_t)std::max<int64_t>(nib_bytes, 16)))) return rc;
    if ((rc = c->nib_src.ensure((size_t)std::max<int64_t>(n, 1) * sizeof(tps_nib_src)))) return rc;
    if (nib_bytes) HIP_TRY(hipMemcpyAsync(c->nib.p, nib, (size_t)nib_bytes, hipMemcpyHostToDevice, c->stream));
    if (n) {
        HIP_TRY(hipMemcpyAsync(c->nib_src.p, src, (size_t)n * sizeof(tps_nib_src), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(sl.desc.p, desc, (size_t)n * sizeof(tps_read_desc), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(tps_pack_kernel_nib4, dim3((unsigned)n), dim3(256), 0, c->stream, (const uint8_t*)c->nib.p,
                           (const tps_nib_src*)c->nib_src.p, (const tps_read_desc*)sl.desc.p, (uint32_t*)sl.seq2.p, (uint16_t*)sl.inv.p, n);
        HIP_TRY(hipGetLastError());
    }
    const bool all_pinned = is_pinned(nib, (size_t)nib_bytes) && is_pinned(src, (size_t)n * sizeof(tps_nib_src)) &&
                            is_pinned(desc, (size_t)n * sizeof(tps_read_desc));
    if (!all_pinned) HIP_TRY(hipStreamSynchronize(c->stream));     // ordinary memory: the copy is over when the call returns
    sl.inv_valid = true;
    sl.any_invalid = flagged;
    reset_slot(sl, n, n_words);
    return TPS_OK;
}

// The kernel family of a fused plan (a.variant = its slide), by table and outputs.
ScanFamily scan_family(const tps::ScanArgs& a, bool want_raw) {
    const bool so = a.pat.so_mask != 0;
    const bool pair = a.pair_n != 0;
    // the default kernels' other slides (sums only, no self-overlap: plan_geometry took the fused path for nothing else)
    if (tps::has_default_only_slide(a.variant)) return (pair && !a.pair16) ? KF_PAIR : KF_PLAIN;
    // sums only, self-overlap table: periods 2 .. 4 have their own kernels (96 registers, 5 waves per SIMD)
    if (so) return want_raw ? (a.lut16 ? KF_SORH : KF_SOR) : (a.pp_d >= 2 && a.pp_d <= 4) ? KF_SOL : KF_SO;
    return want_raw ? KF_RAW : (pair && a.pair16) ? KF_PAIRQ : pair ? KF_PAIR : KF_PLAIN;
}

bool same_params(const tps_params& x, const tps_params& y) { return memcmp(&x, &y, sizeof x) == 0; }

int do_scan(tps_ctx* c, Slot& sl, const tps_params& prm, bool inner = false, hipEvent_t ev_start = nullptr);

// The scan of `sl` at prm.slide = m x base: the fused kernel of the base slide in sl.sub (which borrows the batch), then
// tps_stride_kernel.  Outputs land in sl's buffers in the generic kernel's layout (int32 sums, rows at win_off).
int do_scan_strided(tps_ctx* c, Slot& sl, const tps_params& prm, int base, hipEvent_t ev_a, hipEvent_t ev_b) {
    int rc;
    if (!sl.sub) sl.sub = new Slot();
    Slot& sb = *sl.sub;
    if (sl.sub_stale) {
        sb.seq2.borrow(sl.seq2);
        sb.inv.borrow(sl.inv);
        sb.desc.borrow(sl.desc);
        sb.h_offsets = sl.h_offsets;
        sb.inv_valid = sl.inv_valid;
        sb.any_invalid = sl.any_invalid;
        reset_slot(sb, sl.n, sl.n_words);
        sl.sub_stale = false;
    }
    sb.tails.borrow(sl.tails);
    sb.has_tails = sl.has_tails;
    tps_params pb = prm;
    pb.slide = base;
    pb.flags = (prm.flags | TPS_F_STORE_SUMS) & ~(uint32_t)TPS_F_BINSEG;
    sb.ext_raw = (prm.slide == 2 * base && !c->no_inline_rows) ? sl.args.raw : nullptr;
    sb.ext_raw_win_off = (const int64_t*)sl.win_off.p;
    if ((rc = do_scan(c, sb, pb, true, ev_a))) return rc;
    if (!sb.args.variant) return fail(TPS_E_STATE, "strided scan: the base slide %d did not plan a fused kernel", base);
    const int64_t n = sl.n;
    tps::StrideArgs a{};
    a.base_results = (const tps_read_result*)sb.results.p;
    a.base_sums16 = (const uint16_t*)sb.sums.p;
    a.base_win_off16 = (const int64_t*)sb.win_off16.p;
    a.base_raw = ((prm.flags & TPS_F_STORE_RAW) && !sb.rows_inline) ? (const uint8_t*)sb.raw.p : nullptr;
    a.base_win_off = (const int64_t*)sb.win_off.p;
    a.win_off = (const int64_t*)sl.win_off.p;
    a.sums = sl.args.sums;
    a.raw = sb.rows_inline ? nullptr : sl.args.raw;
    a.results = sl.h_results;
    a.n_reads = n;
    a.m = prm.slide / base;
    a.P = c->pat.P;
    a.n_patterns = c->pat.P;
    a.jump = prm.jump;
    a.min_size = prm.min_size;
    a.binseg = (prm.flags & TPS_F_BINSEG) ? 1 : 0;
    a.s16_dw = (int32_t)((((sl.lay.max_nwin + 1) / 2) + 3) & ~3ll);
    if (a.s16_dw > 3072) a.s16_dw = 0;                 // (12 KB per wave: five workgroups per CU; longer series are read back from HBM)
    const size_t lds = (size_t)tps::WPG * (size_t)(tps::BINSEG_SMEM_DW + a.s16_dw) * 4;
    void* kargs[] = {(void*)&a};
    HIP_TRY(hipExtLaunchKernel((const void*)tps_stride_kernel, dim3((unsigned)((n + tps::WPG - 1) / tps::WPG)), dim3(tps::NT * tps::WPG), kargs, lds, c->stream,
                               nullptr, ev_b, 0));
    // the step-1 counts are the base scan's
    sl.c_start.borrow(sb.c_start);
    sl.c_end.borrow(sb.c_end);
    sl.info_name = std::string(sb.kernel_name) + (a.m == 2 ? " every 2nd window" : a.m == 3 ? " every 3rd window" : " every " + std::to_string(a.m) + "th window");
    sl.kernel_name = sl.info_name.c_str();
    sl.lds_bytes = sb.lds_bytes;
    sl.args.wpg = sb.args.wpg;
    return TPS_OK;
}

// The scan while a wide table is current: one kernel for every slide and flag combination, outputs in the generic kernel's layout
// (results in mapped host memory, c_start / c_end, int32 sums at win_off, u8 rows at win_off * P), so everything downstream is shared.
int do_scan_wide(tps_ctx* c, Slot& sl, const tps_params& prm) {
    int rc;
    const tps_ctx::WideTable& wt = *c->wide_cur;
    const int64_t n = sl.n;
    const int P = wt.P;
    if (!sl.wplanned || !same_params(prm, sl.wplan_prm) || sl.wplan_table != wt.serial) {
        tps::WideArgs w{};
        w.pat = wt.pat;
        const std::string err = tps::plan_wide(w, prm, lds_budget_dw(c));
        if (!err.empty()) return fail(TPS_E_CAPACITY, "%s", err.c_str());
        tps::plan_batch_layout(sl.h_offsets.data(), n, prm, sl.lay);        // (its win_off16 is not used: this kernel writes int32 sums)
        if (c->file_order) sl.lay.order.clear();
        if (!sl.lay.order.empty()) {
            if ((rc = sl.order.ensure((size_t)n * 4))) return rc;
            HIP_TRY(hipMemcpyAsync(sl.order.p, sl.lay.order.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        }
        if ((rc = sl.win_off.ensure((size_t)(n + 1) * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(sl.win_off.p, sl.lay.win_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        sl.wargs = w;
        sl.wplan_prm = prm;
        sl.wplan_table = wt.serial;
        sl.wplanned = true;
    }
    // what the shared downstream calls look at: no fused layout, the wide P, this kernel's name; a later narrow scan plans afresh
    sl.planned = false;
    sl.args = tps::ScanArgs{};
    sl.args.wpg = sl.wargs.wpg;
    sl.plan_p = P;
    sl.plan_k = wt.k;
    sl.stride_base = 0;
    sl.rows_inline = false;
    sl.lds_bytes = (size_t)tps::wide_wg_lds_dwords(sl.wargs) * 4;
    static const char wide_name[] = "tps_scan_kernel_wide";
    sl.kernel_name = wide_name;
    sl.last_flags = prm.flags;
    const int64_t total_win = sl.lay.win_off[(size_t)n];
    if ((rc = ensure_h_results(sl, n))) return rc;
    tps::WideArgs& a = sl.wargs;
    a.seq2 = (const uint32_t*)sl.seq2.p;
    a.inv = (const uint16_t*)sl.inv.p;
    a.desc = (const tps_read_desc*)sl.desc.p;
    a.tails_in = ((prm.flags & TPS_F_TAILS_IN) && !(prm.flags & TPS_F_STEP1)) ? (const uint8_t*)sl.tails.p : nullptr;
    a.img = (const uint32_t*)wt.dev.p;
    a.results = sl.h_results;
    a.c_start = a.c_end = nullptr;
    if (prm.flags & TPS_F_STEP1) {
        if ((rc = sl.c_start.ensure((size_t)std::max<int64_t>(n * P, 1) * 4))) return rc;
        if ((rc = sl.c_end.ensure((size_t)std::max<int64_t>(n * P, 1) * 4))) return rc;
        a.c_start = (int32_t*)sl.c_start.p;
        a.c_end = (int32_t*)sl.c_end.p;
    }
    a.win_off = (const int64_t*)sl.win_off.p;
    a.order = sl.lay.order.empty() ? nullptr : (const int32_t*)sl.order.p;
    a.sums = nullptr;
    a.raw = nullptr;
    if (prm.flags & TPS_F_WINDOWS) {
        if ((rc = sl.sums.ensure((size_t)std::max<int64_t>(total_win, 1) * 4))) return rc;
        a.sums = (int32_t*)sl.sums.p;
    }
    if (prm.flags & TPS_F_STORE_RAW) {
        if ((rc = sl.raw.ensure((size_t)std::max<int64_t>(total_win * P, 1)))) return rc;
        a.raw = (uint8_t*)sl.raw.p;
    }
    a.n_reads = n;
    a.prm = prm;
    if (n == 0) { sl.scanned = true; return TPS_OK; }
    if (c->poison) {
        if ((rc = poison_h_results(c, sl))) return rc;
        if (a.c_start) { TPS_POISON(sl.c_start); TPS_POISON(sl.c_end); }
        if (a.sums) TPS_POISON(sl.sums);
        if (a.raw) TPS_POISON(sl.raw);
    }
    if (sl.lds_bytes > c->lds_set_wide) {
        HIP_TRY(hipFuncSetAttribute((const void*)tps_scan_kernel_wide, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sl.lds_bytes));
        c->lds_set_wide = sl.lds_bytes;
    }
    EventPair ev;
    if ((rc = next_events(c, false, ev))) return rc;
    const int64_t grid = (n + a.wpg - 1) / a.wpg;
    void* kargs[] = {(void*)&a};
    HIP_TRY(hipExtLaunchKernel((const void*)tps_scan_kernel_wide, dim3((unsigned)grid), dim3(tps::NT * a.wpg), kargs, sl.lds_bytes, c->stream,
                               ev.a, ev.b, 0));
    sl.scanned = true;
    return TPS_OK;
}

int do_scan(tps_ctx* c, Slot& sl, const tps_params& prm, bool inner, hipEvent_t ev_start) {
    int rc;
    if (!c->have_pat) return fail(TPS_E_PATTERN, "tps_set_patterns has not been called");
    if ((rc = check_scan(sl, prm))) return rc;
    if (c->wide_cur) return do_scan_wide(c, sl, prm);
    const int64_t n = sl.n;
    const int P = c->pat.P;
    if (!sl.planned || !same_params(prm, sl.plan_prm) || sl.plan_k != c->pat.k || sl.plan_p != P ||
        (sl.plan_dup != 0) != (c->pat.dup_mask != 0) || (sl.plan_so != 0) != (c->pat.so_mask != 0)) {
        tps::plan_batch_layout(sl.h_offsets.data(), n, prm, sl.lay);
        if (c->file_order) sl.lay.order.clear();
        if (!sl.lay.order.empty()) {
            if ((rc = sl.order.ensure((size_t)n * 4))) return rc;
            HIP_TRY(hipMemcpyAsync(sl.order.p, sl.lay.order.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        }
        sl.args = tps::ScanArgs{};
        sl.args.val_on = sl.any_invalid ? 1 : 0;
        if ((rc = plan_lds(c, sl, prm, sl.lay.max_nwin))) return rc;
        sl.stride_base = 0;
        if (!inner && !c->no_stride) {
            sl.stride_base = tps::stride_base(sl.args, prm, c->pat.k, P, [&](int s0) { return window_count(sl.lay.max_len, prm.window, s0, prm.trimfirst, prm.maxlen); },
                                              lds_budget_dw(c), c->knobs);
        }
        if ((rc = sl.win_off.ensure((size_t)(n + 1) * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(sl.win_off.p, sl.lay.win_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        if (sl.args.variant) {                          // fused kernels: the padded layout of their 16-bit sums
            if ((rc = sl.win_off16.ensure((size_t)(n + 1) * 8))) return rc;
            HIP_TRY(hipMemcpyAsync(sl.win_off16.p, sl.lay.win_off16.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));       // sl.lay may be reused by the caller's next plan
        sl.plan_prm = prm;
        sl.plan_k = c->pat.k;
        sl.plan_p = P;
        sl.plan_dup = c->pat.dup_mask;
        sl.plan_so = c->pat.so_mask;
        sl.planned = true;
    }
    const int64_t total_win = sl.lay.win_off[(size_t)n];
    if ((rc = ensure_h_results(sl, n))) return rc;
    tps::ScanArgs& a = sl.args;
    a.seq2 = (const uint32_t*)sl.seq2.p;
    a.inv = (const uint16_t*)sl.inv.p;
    a.desc = (const tps_read_desc*)sl.desc.p;
    a.tails_in = ((prm.flags & TPS_F_TAILS_IN) && !(prm.flags & TPS_F_STEP1)) ? (const uint8_t*)sl.tails.p : nullptr;
    a.lut = (const uint32_t*)c->lut_cur->dev.p;
    a.pair_img = a.lut + (a.pair16 ? c->lut_cur->off_p16 : (a.lut_fields && a.pair_n) ? c->lut_cur->off_pfld : (size_t)a.lut_n);      // (the 32-bit pair table follows the 4^k masks)
    a.lut_img = a.lut + ((a.lut16 && a.lut_fields) ? c->lut_cur->off_f16 : a.lut16 ? c->lut_cur->off_m16 : a.lut_fields ? c->lut_cur->off_fld : c->lut_cur->off_e32);
    a.results = sl.h_results;                      // (written by the kernel straight into mapped pinned host memory)
    if (inner) {                                   // a base-slide scan: its results are read by tps_stride_kernel, not by the host -- they stay in HBM
        if ((rc = sl.results.ensure((size_t)std::max<int64_t>(n, 1) * sizeof(tps_read_result)))) return rc;
        a.results = (tps_read_result*)sl.results.p;
    }
    a.c_start = a.c_end = nullptr;
    if ((prm.flags & TPS_F_STEP1) && !sl.stride_base) {       // (a strided scan borrows the base scan's counts)
        if ((rc = sl.c_start.ensure((size_t)std::max<int64_t>(n * P, 1) * 4))) return rc;
        if ((rc = sl.c_end.ensure((size_t)std::max<int64_t>(n * P, 1) * 4))) return rc;
        a.c_start = (int32_t*)sl.c_start.p;
        a.c_end = (int32_t*)sl.c_end.p;
    }
    a.win_off = (const int64_t*)sl.win_off.p;
    a.order = sl.lay.order.empty() ? nullptr : (const int32_t*)sl.order.p;
    a.sums = nullptr;
    a.sums16 = nullptr;
    a.win_off16 = nullptr;
    a.raw = nullptr;
    if (prm.flags & TPS_F_WINDOWS) {
        // S_w always goes to HBM: it is the step's output and the only copy the exact change-point fallback can re-read;
        // TPS_F_STORE_SUMS just makes it downloadable.  The fused kernels write 16-bit values (2 B per window, every read
        // padded to 8 windows), the generic kernel int32; tps_batch_window_sums hands out int32 either way.
        if (a.variant) {
            if ((rc = sl.sums.ensure((size_t)std::max<int64_t>(sl.lay.win_off16[(size_t)n], 8) * 2))) return rc;
            a.sums16 = (uint16_t*)sl.sums.p;
            a.win_off16 = (const int64_t*)sl.win_off16.p;
        } else {
            if ((rc = sl.sums.ensure((size_t)std::max<int64_t>(total_win, 1) * 4))) return rc;
            a.sums = (int32_t*)sl.sums.p;
        }
    }
    a.raw_m = 0;
    a.raw_win_off = nullptr;
    sl.rows_inline = false;
    if (prm.flags & TPS_F_STORE_RAW) {
        // a base-slide scan at half the requested slide: the per-pattern tiles store the even windows' rows straight into the requesting
        // scan's layout (rows of whole dwords; a clean batch -- the fallback tile of a batch with non-ACGT letters writes whole rows by
        // address; the self-overlap tiles' repairs follow the same mapping)
        if (inner && sl.ext_raw && a.variant && a.pp_d >= 0 && (c->pat.so_mask == 0 ? a.pp_d == 0 : a.pp_d > 0) && (P & 3) == 0 && !sl.any_invalid) {
            a.raw = (uint8_t*)sl.ext_raw;
            a.raw_m = 2;
            a.raw_win_off = sl.ext_raw_win_off;
            sl.rows_inline = true;
        } else {
            if ((rc = sl.raw.ensure((size_t)std::max<int64_t>(total_win * P, 1)))) return rc;
            a.raw = (uint8_t*)sl.raw.p;
        }
    }
    a.lc_scratch = nullptr;
    if (a.lc_global) {
        if ((rc = sl.lc.ensure((size_t)std::max<int64_t>(n, 1) * (size_t)a.lc_stride * 2))) return rc;
        a.lc_scratch = (uint16_t*)sl.lc.p;
    }
    if (c->poison) {
        // everything this scan writes or uses as scratch; borrowed buffers (a strided scan's base counts) and the rows an inner scan
        // stores into the requesting scan's layout (ext_raw: that scan filled its own buffer before it came here) are left alone
        if (inner) TPS_POISON(sl.results);
        else if ((rc = poison_h_results(c, sl))) return rc;
        if (a.c_start) { TPS_POISON(sl.c_start); TPS_POISON(sl.c_end); }
        if (a.sums || a.sums16) TPS_POISON(sl.sums);
        if (a.raw && !sl.rows_inline) TPS_POISON(sl.raw);
        if (a.lc_scratch) TPS_POISON(sl.lc);
    }
    a.stamps = nullptr;
    if (c->want_stamps) {
        if ((rc = sl.stamps.ensure((size_t)std::max<int64_t>(n, 1) * 16 * 8))) return rc;
        TPS_POISON(sl.stamps);
        HIP_TRY(hipMemsetAsync(sl.stamps.p, 0, (size_t)std::max<int64_t>(n, 1) * 16 * 8, c->stream));
        a.stamps = (uint64_t*)sl.stamps.p;
    }
    a.n_reads = n;
    a.pat = c->pat;
    a.prm = prm;
    sl.last_flags = prm.flags;
    if (n == 0) { sl.scanned = true; return TPS_OK; }

    // which kernel the plan launches: the generic one, or the fused kernel of its slide and family
    const ScanKernel* k = &GENERIC_KERNEL;
    size_t* lds_set = &c->lds_set_generic;
    if (tps::has_specialised_slide(a.variant) || tps::has_default_only_slide(a.variant)) {
        const ScanFamily fam = scan_family(a, a.raw != nullptr);
        k = &FUSED_KERNELS[fam][a.variant - KSLIDE_MIN];
        lds_set = &c->lds_set_fused[fam][a.variant - KSLIDE_MIN];
    }
    sl.kernel_name = k->name;
    if (sl.lds_bytes > *lds_set) {
        HIP_TRY(hipFuncSetAttribute(k->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sl.lds_bytes));
        *lds_set = sl.lds_bytes;
    }
    EventPair ev;
    if ((rc = next_events(c, inner, ev))) return rc;
    if (sl.stride_base) {
        // (timed from the base kernel's start to the end of the compaction + change-point kernel)
        if ((rc = do_scan_strided(c, sl, prm, sl.stride_base, ev.a, ev.b))) return rc;
        sl.scanned = true;
        return TPS_OK;
    }
    {
        // hipExtLaunchKernel stamps the pair of events from the dispatch packet's own start / end timestamps:
        // no separate barrier packets around the kernel (two hipEventRecord calls cost ~6 us per launch and
        // kept consecutive launches from running back to back)
        const int64_t grid = (n + a.wpg - 1) / a.wpg;
        void* kargs[] = {(void*)&a};
        HIP_TRY(hipExtLaunchKernel(k->fn, dim3((unsigned)grid), dim3(tps::NT * a.wpg), kargs, sl.lds_bytes, c->stream,
                                   inner ? ev_start : ev.a, ev.b, 0));
    }
    sl.scanned = true;
    return TPS_OK;
}

Slot* get_slot(tps_ctx* c, int slot) {
    if (!c || slot < 0 || slot >= TPS_MAX_SLOTS) { fail(TPS_E_ARG, "slot out of range"); return nullptr; }
    return &c->slots[slot];
}

// ---- the steps the read-analysis calls share (tps_batch_kmer_followers .. tps_batch_mod_profile; DESIGN.md, "How a read-analysis
// call is put together").  Each call: need_batch (or bind alone, where it takes no batch), its check function from the feature's
// header, its layouts (tps_layout.h), ensure + TPS_POISON, its clearing memsets and input copies, launch_waves, download.

// bind and the slot; ... and a batch in it (the sibling of need_scanned below)
int need_slot(tps_ctx* c, int slot, Slot** out) {
    int rc;
    if ((rc = bind(c))) return rc;
    return (*out = get_slot(c, slot)) ? TPS_OK : TPS_E_ARG;
}
int have_batch(const Slot& sl) { return sl.n < 0 ? fail(TPS_E_STATE, "no batch uploaded in this slot") : TPS_OK; }
int need_batch(tps_ctx* c, int slot, Slot** out) {
    int rc;
    if ((rc = need_slot(c, slot, out))) return rc;
    return have_batch(**out);
}

// the slot's packed batch in a kernel's arguments
template <class A>
void set_batch(A& a, const Slot& sl) {
    a.seq2 = (const uint32_t*)sl.seq2.p;
    a.inv = (const uint16_t*)sl.inv.p;
    a.desc = (const tps_read_desc*)sl.desc.p;
}

// piece `off` of a device buffer laid out with tps::Layout
template <class T>
T* at(const DevBuf& b, size_t off) { return (T*)((char*)b.p + off); }

// tails / begin / end of n reads into `buf` where region_layout put them, and into the kernel's arguments
template <class A>
int upload_region(tps_ctx* c, const DevBuf& buf, const tps::RegionAt& r, const uint8_t* tails, const int32_t* begin, const int32_t* end, int64_t n, A& a) {
    a.tails = at<const uint8_t>(buf, r.tails);
    a.begin = at<const int32_t>(buf, r.begin);
    a.end = at<const int32_t>(buf, r.end);
    HIP_TRY(hipMemcpyAsync((void*)a.tails, tails, (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.begin, begin, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.end, end, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    return TPS_OK;
}

// The telomere hit table of (unit, m), built into `table` and copied to c->tract_table; *w = the letters of its words.  `table` is the
// CALLER's local: the copy is from pageable memory and has left it when the call returns -- every call ends in download(), which
// waits for the stream -- so it must live that long, not just as long as this function.
int upload_hit_table(tps_ctx* c, uint64_t unit, int m, std::vector<uint32_t>& table, int* w) {
    int rc;
    *w = m < tps::TRACT_MAX_WORD ? m : tps::TRACT_MAX_WORD;
    table.resize((size_t)tps::tract_table_dw(*w));
    tps::tract_hit_table(unit, m, table.data());
    if ((rc = c->tract_table.ensure(table.size() * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(c->tract_table.p, table.data(), table.size() * 4, hipMemcpyHostToDevice, c->stream));
    return TPS_OK;
}

// one wave per read (or row), wpg waves per workgroup; lds_bytes: the dynamic LDS of a kernel that has some
template <class A>
int launch_waves(tps_ctx* c, void (*kernel)(A), int64_t n, int wpg, const A& a, size_t lds_bytes = 0) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + wpg - 1) / wpg)), dim3(tps::NT * wpg), lds_bytes, c->stream, a);
    HIP_TRY(hipGetLastError());
    return TPS_OK;
}

// the outputs back to the host (a piece without a host pointer was not asked for), then the wait for the stream
struct Down { void* host; const void* dev; size_t bytes; };
int download(tps_ctx* c, std::initializer_list<Down> parts) {
    for (const Down& d : parts)
        if (d.host) HIP_TRY(hipMemcpyAsync(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return TPS_OK;
}

}  // namespace

// ======================================================================== C ABI
extern "C" {

int tps_abi_version(void) { return TPS_ABI_VERSION; }

const char* tps_last_error(void) { return g_err.c_str(); }

int tps_device_count(int* n) {
    if (!n) return fail(TPS_E_ARG, "null pointer");
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess) { *n = 0; return fail(TPS_E_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *n = cnt;
    return TPS_OK;
}

int tps_ctx_create(int device, tps_ctx** out) {
    if (!out) return fail(TPS_E_ARG, "null pointer");
    *out = nullptr;
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0)
        return fail(TPS_E_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= cnt) return fail(TPS_E_NO_DEVICE, "device %d out of range (0..%d)", device, cnt - 1);
    tps_ctx* c = new tps_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&c->prop, device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(TPS_E_HIP, "cannot initialise device %d", device);
    }
    *out = c;
    return TPS_OK;
}

int tps_ctx_destroy(tps_ctx* c) {
    if (!c) return TPS_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (void* hp : c->pinned) {
        { std::lock_guard<std::mutex> lk(g_pinned_mu); g_pinned.erase((uintptr_t)hp); }
        (void)hipHostFree(hp);
    }
    if (c->h_flag) (void)hipHostFree(c->h_flag);
    if (c->share_ev) (void)hipEventDestroy(c->share_ev);
    for (int i = 0; i < 2; ++i) {
        if (c->raw_stage[i]) (void)hipHostFree(c->raw_stage[i]);
        if (c->raw_ev[i]) (void)hipEventDestroy(c->raw_ev[i]);
    }
    c->pinned.clear();
    for (auto& ep : c->ev_pool) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
    (void)hipStreamDestroy(c->stream);
    delete c;                                      // (device buffers go with what holds them: DevBuf, Slot)
    return TPS_OK;
}

int tps_device_info(tps_ctx* c, char* buf, int32_t buf_len) {
    if (!c || !buf || buf_len < 1) return fail(TPS_E_ARG, "bad arguments");
    snprintf(buf, (size_t)buf_len, "%s arch=%s CUs=%d LDS/block=%zu clock=%dkHz pci=%04x:%02x:%02x", c->prop.name, c->prop.gcnArchName,
             c->prop.multiProcessorCount, c->prop.sharedMemPerBlock, c->prop.clockRate, c->prop.pciDomainID, c->prop.pciBusID, c->prop.pciDeviceID);
    return TPS_OK;
}

int tps_batch_kernel_info(tps_ctx* c, int32_t slot, char* buf, int32_t buf_len) {
    if (!c || !buf || buf_len < 1) return fail(TPS_E_ARG, "bad arguments");
    Slot* sl = get_slot(c, slot);
    if (!sl) return TPS_E_ARG;
    if (!sl->scanned) return fail(TPS_E_STATE, "slot %d has not been scanned", slot);
    const size_t gran = (sl->lds_bytes + 1279) / 1280;
    const int wgs = gran ? (int)std::min<size_t>(128 / gran, 8) : 8;
    snprintf(buf, (size_t)buf_len, "%s lds=%zu wgs_per_cu=%d waves_per_wg=%d", sl->kernel_name, sl->lds_bytes, wgs, sl->args.wpg);
    return TPS_OK;
}

int tps_set_patterns(tps_ctx* c, const char* pats, int32_t P, int32_t k) {
    int rc;
    if ((rc = bind(c))) return rc;
    if (!pats) return fail(TPS_E_ARG, "null pattern table");
    if (P < 1 || k < 1 || P > TPS_MAX_PATTERNS || k > TPS_MAX_K) return fail(TPS_E_PATTERN, "%d patterns of %d letters not supported", P, k);
    // a few tables stay resident (a multi-k run switches between them once per batch and k: no copy, no sync)
    const std::string key(pats, (size_t)P * (size_t)k);
    for (auto& t : c->tables)
        if (t.P == P && t.k == k && t.key == key) {
            c->lut_cur = &t;
            c->pat = t.pat;
            c->have_pat = true;
            c->wide_cur = nullptr;
            drop_plans(c);
            return TPS_OK;
        }
    std::vector<uint32_t> lut;
    tps::PatInfo pi{};
    std::string err = tps::build_patterns(pats, P, k, lut, pi);
    if (!err.empty()) return fail(TPS_E_PATTERN, "%s", err.c_str());
    if (k <= 4) {
        // pair table for the pair kernels (k <= 4, see plan_geometry): entry of the (k+1)-mer code c =
        // packed entries (mask << 16 | popcount) of the k-mers at p and p+1, masks ORed, counts added
        const size_t n1 = lut.size(), n2 = n1 * 4;
        const uint32_t km = (uint32_t)n1 - 1u;
        lut.resize(n1 + n2);
        for (size_t cc = 0; cc < n2; ++cc) {
            const uint32_t m1 = lut[cc & km], m2 = lut[(cc >> 2) & km];
            lut[n1 + cc] = ((m1 | m2) << 16) | (uint32_t)(__builtin_popcount(m1) + __builtin_popcount(m2));
        }
    }
    size_t off_e32 = 0, off_fld = 0, off_m16 = 0, off_f16 = 0, off_p16 = 0, off_pfld = 0;
    if (!pi.hash_shift) {
        const size_t n1 = (size_t)1 << (2 * k), n4 = (n1 + 3) & ~(size_t)3, n16 = ((n1 + 1) / 2 + 3) & ~(size_t)3;
        off_e32 = (lut.size() + 3) & ~(size_t)3;       // (16-byte aligned: the kernels copy uint4)
        off_fld = off_e32 + n4;
        off_m16 = off_fld + n4;
        off_f16 = off_m16 + n16;
        lut.resize(off_f16 + n16, 0u);
        for (size_t i = 0; i < n1; ++i) {
            const uint32_t m = lut[i];
            lut[off_e32 + i] = (m << 16) | (uint32_t)__builtin_popcount(m);
            lut[off_fld + i] = tps::mask_to_fields(m);
            ((uint16_t*)&lut[off_m16])[i] = (uint16_t)m;
            // (field index of THE pattern: tables with duplicate k-mers never take the kernels that read this image)
            ((uint16_t*)&lut[off_f16])[i] = m ? (uint16_t)(1u << tps::pp_field(__builtin_ctz(m))) : (uint16_t)0;
        }
        if (k <= 4) {
            // pair table of one-hot FIELDS for the raw-row kernels' per-pattern tiles (tile_pp_s<.., PAIRF>): entry of the (k+1)-mer
            // code c = field of the k-mer at p + field of the one at p + 1
            const size_t n2 = n1 * 4;
            off_pfld = lut.size();                      // (a multiple of 4 dwords)
            lut.resize(off_pfld + n2, 0u);
            for (size_t cc = 0; cc < n2; ++cc) lut[off_pfld + cc] = lut[off_fld + (cc & (n1 - 1))] + lut[off_fld + ((cc >> 2) & (n1 - 1))];
        }
        if (k == 5 && P <= 16) {
            // 16-bit pair table of the _s*q kernels (ScanArgs::pair16): entry of the (k+1)-mer code c = the masks of the k-mers at p
            // and p + 1 ORed (counts are popcounts: the planner takes it for tables without self-overlap only)
            const size_t n2 = n1 * 4;
            off_p16 = lut.size();                       // (a multiple of 4 dwords)
            lut.resize(off_p16 + n2 / 2, 0u);
            for (size_t cc = 0; cc < n2; ++cc)
                ((uint16_t*)&lut[off_p16])[cc] = (uint16_t)(lut[cc & (n1 - 1)] | lut[(cc >> 2) & (n1 - 1)]);
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));          // no launch may still be reading the table that gets recycled
    tps_ctx::Table* slot = nullptr;
    if (c->tables.size() < 6) { c->tables.emplace_back(); slot = &c->tables.back(); }
    else { slot = &c->tables[c->table_rr++ % c->tables.size()]; }
    if ((rc = slot->dev.ensure(lut.size() * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(slot->dev.p, lut.data(), lut.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    slot->P = P; slot->k = k; slot->key = key; slot->pat = pi;
    slot->off_e32 = off_e32; slot->off_fld = off_fld; slot->off_m16 = off_m16; slot->off_f16 = off_f16; slot->off_p16 = off_p16; slot->off_pfld = off_pfld;
    c->lut_cur = slot;
    c->pat = pi;
    c->have_pat = true;
    c->wide_cur = nullptr;
    drop_plans(c);                                     // kernel choice and LDS plan depend on the table (periods, duplicates, k)
    return TPS_OK;
}

int tps_set_patterns_wide(tps_ctx* c, const char* pats, int32_t P, int32_t k) {
    int rc;
    if ((rc = bind(c))) return rc;
    if (!pats) return fail(TPS_E_ARG, "null pattern table");
    if (P < 1 || k < 1 || P > TPS_WIDE_MAX_PATTERNS || k > TPS_WIDE_MAX_K) return fail(TPS_E_PATTERN, "%d patterns of %d letters not supported", P, k);
    const std::string key(pats, (size_t)P * (size_t)k);
    tps_ctx::WideTable* cur = nullptr;
    for (auto& t : c->wtables)
        if (t.P == P && t.k == k && t.key == key) cur = &t;
    if (!cur) {
        std::vector<uint32_t> img;
        tps::WidePat wp{};
        const std::string err = tps::build_wide_table(pats, P, k, img, wp);
        if (!err.empty()) return fail(TPS_E_PATTERN, "%s", err.c_str());
        HIP_TRY(hipStreamSynchronize(c->stream));          // no launch may still be reading the table that gets recycled
        if (c->wtables.size() < 6) { c->wtables.emplace_back(); cur = &c->wtables.back(); }
        else { cur = &c->wtables[c->wtable_rr++ % c->wtables.size()]; }
        if ((rc = cur->dev.ensure(img.size() * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(cur->dev.p, img.data(), img.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        cur->P = P; cur->k = k; cur->key = key; cur->pat = wp;
        cur->serial = ++c->table_serial;
    }
    c->wide_cur = cur;
    c->pat = tps::PatInfo{};                           // (what the shared host code reads of the narrow table's description: P and k)
    c->pat.P = P;
    c->pat.k = k;
    c->have_pat = true;
    drop_plans(c);
    return TPS_OK;
}

int tps_batch_upload(tps_ctx* c, int32_t slot, const uint8_t* bases, const int64_t* offsets, int64_t n) {
    int rc;
    if ((rc = bind(c))) return rc;
    Slot* sl = get_slot(c, slot);
    if (!sl) return TPS_E_ARG;
    return do_upload(c, *sl, bases, offsets, n);
}

int tps_batch_upload_packed(tps_ctx* c, int32_t slot, const uint32_t* seq2, const uint16_t* inv, const tps_read_desc* desc,
                            int64_t n, int64_t n_words) {
    int rc;
    if ((rc = bind(c))) return rc;
    Slot* sl = get_slot(c, slot);
    if (!sl) return TPS_E_ARG;
    return do_upload_packed(c, *sl, seq2, inv, desc, n, n_words);
}

int tps_batch_upload_nib4(tps_ctx* c, int32_t slot, const uint8_t* nib, int64_t nib_bytes, const tps_nib_src* src, const tps_read_desc* desc,
                          int64_t n, int64_t n_words) {
    int rc;
    if ((rc = bind(c))) return rc;
    Slot* sl = get_slot(c, slot);
    if (!sl) return TPS_E_ARG;
    return do_upload_nib4(c, *sl, nib, nib_bytes, src, desc, n, n_words);
}

int tps_batch_share(tps_ctx* c, int32_t slot, tps_ctx* src, int32_t src_slot) {
    int rc;
    if ((rc = bind(c))) return rc;
    if (!src || src == c) return fail(TPS_E_ARG, "the batch must come from another context");
    if (src->device != c->device) return fail(TPS_E_ARG, "both contexts must be on the same device (%d vs %d)", c->device, src->device);
    Slot* sl = get_slot(c, slot);
    Slot* from = get_slot(src, src_slot);
    if (!sl || !from) return TPS_E_ARG;
    if (from->n < 0) return fail(TPS_E_STATE, "no batch uploaded in the source slot");
    // whatever this context still has in flight on the slot's old buffers must be over before they are let go
    HIP_TRY(hipStreamSynchronize(c->stream));
    sl->seq2.borrow(from->seq2);
    sl->inv.borrow(from->inv);
    sl->desc.borrow(from->desc);
    sl->h_offsets = from->h_offsets;
    sl->inv_valid = from->inv_valid;
    sl->any_invalid = from->any_invalid;
    reset_slot(*sl, from->n, from->n_words);
    // the source's upload may still be running on ITS stream: this context's stream waits for it
    if (!c->share_ev) HIP_TRY(hipEventCreateWithFlags(&c->share_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->share_ev, src->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->share_ev, 0));
    return TPS_OK;
}

int tps_host_alloc(tps_ctx* c, int64_t bytes, void** out) {
    int rc;
    if ((rc = bind(c))) return rc;
    if (!out || bytes < 0) return fail(TPS_E_ARG, "bad arguments");
    *out = nullptr;
    void* p = nullptr;
    HIP_TRY(hipHostMalloc(&p, (size_t)std::max<int64_t>(bytes, 16), hipHostMallocPortable));
    c->pinned.insert(p);
    { std::lock_guard<std::mutex> lk(g_pinned_mu); g_pinned[(uintptr_t)p] = (size_t)std::max<int64_t>(bytes, 16); }
    *out = p;
    return TPS_OK;
}

int tps_host_free(tps_ctx* c, void* p) {
    int rc;
    if ((rc = bind(c))) return rc;
    if (!p) return TPS_OK;
    if (!c->pinned.erase(p)) return fail(TPS_E_ARG, "pointer was not allocated by tps_host_alloc of this context");
    { std::lock_guard<std::mutex> lk(g_pinned_mu); g_pinned.erase((uintptr_t)p); }
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipHostFree(p));
    return TPS_OK;
}

int tps_batch_download_packed(tps_ctx* c, int32_t slot, uint32_t* seq2, uint16_t* inv, tps_read_desc* desc, int64_t n, int64_t n_words,
                              int64_t* n_words_out) {
    int rc;
    if ((rc = bind(c))) return rc;
    Slot* sl = get_slot(c, slot);
    if (!sl) return TPS_E_ARG;
    if (sl->n < 0) return fail(TPS_E_STATE, "no batch uploaded in this slot");
    if (n_words_out) *n_words_out = sl->n_words;
    if ((seq2 || inv) && n_words != sl->n_words) return fail(TPS_E_ARG, "buffers must hold %lld words", (long long)sl->n_words);
    if (desc && n != sl->n) return fail(TPS_E_ARG, "desc must hold %lld reads", (long long)sl->n);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (seq2 && n_words) HIP_TRY(hipMemcpy(seq2, sl->seq2.p, (size_t)n_words * 4, hipMemcpyDeviceToHost));
    if (inv && n_words) {
        if (!sl->inv_valid) memset(inv, 0, (size_t)n_words * 2);
        else HIP_TRY(hipMemcpy(inv, sl->inv.p, (size_t)n_words * 2, hipMemcpyDeviceToHost));
    }
    if (desc && n) HIP_TRY(hipMemcpy(desc, sl->desc.p, (size_t)n * sizeof(tps_read_desc), hipMemcpyDeviceToHost));
    return TPS_OK;
}

int tps_batch_kmer_followers(tps_ctx* c, int32_t slot, int32_t n_fwd, int32_t follow, int32_t lo, int32_t hi, int32_t min_len,
                             uint32_t* picks, int64_t picks_words, int64_t* hist, int64_t hist_len) {
    int rc;
    Slot* sl;
    tps::Why why;
    if ((rc = need_slot(c, slot, &sl))) return rc;
    if (!c->have_pat) return fail(TPS_E_PATTERN, "tps_set_patterns has not been called");
    if (c->wide_cur) return fail(TPS_E_PATTERN, "tps_batch_kmer_followers does not take a wide pattern table (n_fwd <= 15: set the table with tps_set_patterns)");
    if ((rc = have_batch(*sl))) return rc;
    const int64_t n = sl->n;
    if ((rc = tps::followers_check(c->pat.P, n, n_fwd, follow, lo, hi, picks, picks_words, hist, hist_len, &why))) return fail(rc, "%s", why.msg);
    if (n == 0) { if (hist) memset(hist, 0, (size_t)hist_len * 8); return TPS_OK; }
    const int pw = (hi - lo + 31) / 32, nbins = (1 << (2 * follow)) + 1;
    const size_t picks_bytes = (size_t)picks_words * 4, hist_bytes = (size_t)2 * n_fwd * nbins * 8;
    // scratch: the slot's raw / sums buffers are not touched; picks and counters get buffers of their own in the context
    if ((rc = c->follow_picks.ensure(picks_bytes))) return rc;
    if ((rc = c->follow_hist.ensure(hist_bytes))) return rc;
    TPS_POISON(c->follow_picks);
    TPS_POISON(c->follow_hist);
    HIP_TRY(hipMemsetAsync(c->follow_picks.p, 0, picks_bytes, c->stream));
    HIP_TRY(hipMemsetAsync(c->follow_hist.p, 0, hist_bytes, c->stream));
    tps::FollowArgs a{};
    set_batch(a, *sl);
    a.lut = (const uint32_t*)c->lut_cur->dev.p;
    a.picks = (uint32_t*)c->follow_picks.p;
    a.hist = hist ? (unsigned long long*)c->follow_hist.p : nullptr;
    a.n_reads = n;
    a.pat = c->pat;
    a.n_fwd = n_fwd; a.follow = follow; a.lo = lo; a.hi = hi; a.min_len = min_len; a.pw = pw; a.nbins = nbins;
    if ((rc = launch_waves(c, tps_followers_kernel, n, tps::WPG, a))) return rc;
    return download(c, {{picks, a.picks, picks_bytes}, {hist, c->follow_hist.p, hist_bytes}});
}

int tps_batch_kmer_followers_wide(tps_ctx* c, int32_t slot, int32_t n_fwd, int32_t follow, int32_t lo, int32_t hi, int32_t min_len,
                                  uint32_t* picks, int64_t picks_words, int64_t* hist, int64_t hist_len) {
    int rc;
    Slot* sl;
    tps::Why why;
    if ((rc = need_slot(c, slot, &sl))) return rc;
    if (!c->have_pat || !c->wide_cur) return fail(TPS_E_PATTERN, "tps_batch_kmer_followers_wide needs a table set with tps_set_patterns_wide");
    if ((rc = have_batch(*sl))) return rc;
    // (static LDS of at most 64 KB: the 160 KB cap of lds_budget_dw never decides here.  The assertion restates the sum of
    // followers_wide_wg_lds_dwords(), which is not constexpr; should the two drift apart, the kernel's own static array, sized by
    // the same constants, still refuses to compile beyond 64 KB)
    static_assert((tps::WIDE_IMG_DW + tps::WPG * tps::FOLLOWW_LDS_DW) * 4 <= 64 * 1024, "tps_followers_kernel_wide: followers_wide_wg_lds_dwords() within every device's budget cap");
    if (tps::followers_wide_wg_lds_dwords() > lds_budget_dw(c))
        return fail(TPS_E_CAPACITY, "the wide followers kernel needs %lld bytes of LDS per workgroup", (long long)tps::followers_wide_wg_lds_dwords() * 4);
    const tps_ctx::WideTable& wt = *c->wide_cur;
    const int64_t n = sl->n;
    if ((rc = tps::followers_wide_check(wt.P, n, n_fwd, follow, lo, hi, picks, picks_words, hist, hist_len, &why))) return fail(rc, "%s", why.msg);
    if (n == 0) { if (hist) memset(hist, 0, (size_t)hist_len * 8); return TPS_OK; }
    const int pw = (hi - lo + 31) / 32, nbins = hist ? (1 << (2 * follow)) + 1 : 0;
    const size_t picks_bytes = (size_t)picks_words * 4, hist_bytes = (size_t)hist_len * 8;
    if ((rc = c->follow_picks.ensure(picks_bytes))) return rc;
    TPS_POISON(c->follow_picks);
    HIP_TRY(hipMemsetAsync(c->follow_picks.p, 0, picks_bytes, c->stream));
    if (hist) {
        if ((rc = c->follow_hist.ensure(hist_bytes))) return rc;
        TPS_POISON(c->follow_hist);
        HIP_TRY(hipMemsetAsync(c->follow_hist.p, 0, hist_bytes, c->stream));
    }
    tps::FollowWideArgs a{};
    set_batch(a, *sl);
    a.img = (const uint32_t*)wt.dev.p;
    a.picks = (uint32_t*)c->follow_picks.p;
    a.hist = hist ? (unsigned long long*)c->follow_hist.p : nullptr;
    a.n_reads = n;
    a.pat = wt.pat;
    a.n_fwd = n_fwd; a.follow = follow; a.lo = lo; a.hi = hi; a.min_len = min_len; a.pw = pw; a.nbins = nbins;
    if ((rc = launch_waves(c, tps_followers_kernel_wide, n, tps::WPG, a))) return rc;
    return download(c, {{picks, a.picks, picks_bytes}, {hist, c->follow_hist.p, hist_bytes}});
}

int tps_batch_motif_census(tps_ctx* c, int32_t slot, int32_t u_min, int32_t u_max, int32_t lo, int32_t hi, int32_t min_len,
                           tps_motif_hit* hits, int64_t n_hits, int32_t* counts, int64_t counts_len) {
    int rc;
    Slot* sl;
    tps::Why why;
    if ((rc = need_batch(c, slot, &sl))) return rc;
    const int64_t n = sl->n;
    if ((rc = tps::motif_census_check(n, u_min, u_max, lo, hi, hits, n_hits, counts, counts_len, &why))) return fail(rc, "%s", why.msg);
    if (n == 0) return TPS_OK;
    // (the table, the slot's scan outputs and its plan are not touched: a scan before and after the census gives the same results)
    const size_t hit_bytes = (size_t)n * 2 * sizeof(tps_motif_hit), cnt_bytes = (size_t)n * 2 * (u_max - u_min + 1) * 4;
    if ((rc = c->motif_hits.ensure(hit_bytes))) return rc;
    TPS_POISON(c->motif_hits);
    HIP_TRY(hipMemsetAsync(c->motif_hits.p, 0, hit_bytes, c->stream));
    if (counts) {
        if ((rc = c->motif_counts.ensure(cnt_bytes))) return rc;
        TPS_POISON(c->motif_counts);
        HIP_TRY(hipMemsetAsync(c->motif_counts.p, 0, cnt_bytes, c->stream));
    }
    tps::MotifArgs a{};
    set_batch(a, *sl);
    a.hits = (tps_motif_hit*)c->motif_hits.p;
    a.counts = counts ? (int32_t*)c->motif_counts.p : nullptr;
    a.n_reads = n;
    a.u_min = u_min; a.u_max = u_max; a.lo = lo; a.hi = hi; a.min_len = min_len;
    if ((rc = launch_waves(c, tps::motif_census_kernel, n, tps::WPG, a))) return rc;
    return download(c, {{hits, a.hits, hit_bytes}, {counts, c->motif_counts.p, cnt_bytes}});
}

int tps_batch_variant_census(tps_ctx* c, int32_t slot, uint64_t unit, int32_t m, const uint8_t* tails, const int32_t* begin, const int32_t* end,
                             int64_t n_reads, int32_t bin, int32_t n_bins, uint32_t* counts, int64_t counts_len, int64_t* profile, int64_t profile_len) {
    int rc;
    Slot* sl;
    tps::Why why;
    if ((rc = need_batch(c, slot, &sl))) return rc;
    const int64_t n = sl->n;
    if ((rc = tps::variant_census_check(n, unit, m, tails, begin, end, n_reads, bin, n_bins, counts, counts_len, profile, profile_len, &why)))
        return fail(rc, "%s", why.msg);
    if (profile) memset(profile, 0, (size_t)profile_len * 8);
    if (n == 0) return TPS_OK;
    // (the table, the slot's tails, its scan outputs and its plan are not touched: a scan before and after the census gives the same results)
    const int cols = 2 + 4 * m;
    const size_t cnt_bytes = (size_t)n * cols * 4, part_len = (size_t)n_bins * cols, prof_bytes = tps::VARIANT_PARTS * part_len * 8;
    tps::Layout in;
    const tps::RegionAt reg = tps::region_layout(in, n);
    if ((rc = c->variant_in.ensure(in.total))) return rc;
    if ((rc = c->variant_counts.ensure(cnt_bytes))) return rc;
    TPS_POISON(c->variant_counts);
    tps::VariantArgs a{};
    set_batch(a, *sl);
    if ((rc = upload_region(c, c->variant_in, reg, tails, begin, end, n, a))) return rc;
    HIP_TRY(hipMemsetAsync(c->variant_counts.p, 0, cnt_bytes, c->stream));
    if (profile) {
        if ((rc = c->variant_prof.ensure(prof_bytes))) return rc;
        TPS_POISON(c->variant_prof);
        HIP_TRY(hipMemsetAsync(c->variant_prof.p, 0, prof_bytes, c->stream));
        c->h_variant_prof.resize(tps::VARIANT_PARTS * part_len);
    }
    a.counts = (uint32_t*)c->variant_counts.p;
    a.prof = profile ? (unsigned long long*)c->variant_prof.p : nullptr;
    a.n_reads = n;
    a.unit = unit; a.m = m; a.bin = bin; a.n_bins = n_bins;
    if ((rc = launch_waves(c, tps::variant_census_kernel, n, tps::WPG, a))) return rc;
    if ((rc = download(c, {{counts, a.counts, cnt_bytes}, {profile ? c->h_variant_prof.data() : nullptr, c->variant_prof.p, prof_bytes}}))) return rc;
    if (profile)
        for (int p = 0; p < tps::VARIANT_PARTS; ++p)
            for (size_t i = 0; i < part_len; ++i) profile[i] += (int64_t)c->h_variant_prof[p * part_len + i];
    return TPS_OK;
}

int tps_batch_tract_map(tps_ctx* c, int32_t slot, uint64_t unit, int32_t m, int32_t block, int32_t min_hits, int32_t gap, int32_t min_blocks,
                        int32_t max_tracts, tps_tract* tracts, int64_t tracts_len, int32_t* found, int64_t found_len, uint32_t* totals, int64_t totals_len) {
    int rc, w;
    Slot* sl;
    tps::Why why;
    if ((rc = need_batch(c, slot, &sl))) return rc;
    const int64_t n = sl->n;
    if ((rc = tps::tract_map_check(n, unit, m, block, min_hits, gap, min_blocks, max_tracts, tracts, tracts_len, found, found_len, totals, totals_len, &why)))
        return fail(rc, "%s", why.msg);
    if (n == 0) return TPS_OK;
    // (the pattern table, the slot's tails, its scan outputs and its plan are not touched: a scan before and after the map gives the same results)
    tps::Layout out;
    const size_t tr_bytes = (size_t)n * 2 * max_tracts * sizeof(tps_tract), fo_bytes = (size_t)n * 2 * 4, to_bytes = (size_t)n * 4 * 4;
    const size_t off_tr = out.add(tr_bytes), off_fo = out.add(fo_bytes), off_to = out.add(to_bytes);
    if ((rc = c->tract_out.ensure(out.total))) return rc;
    TPS_POISON(c->tract_out);
    std::vector<uint32_t> table;
    if ((rc = upload_hit_table(c, unit, m, table, &w))) return rc;
    HIP_TRY(hipMemsetAsync(c->tract_out.p, 0, out.total, c->stream));
    tps::TractArgs a{};
    set_batch(a, *sl);
    a.table = (const uint32_t*)c->tract_table.p;
    a.tracts = at<tps_tract>(c->tract_out, off_tr);
    a.found = at<int32_t>(c->tract_out, off_fo);
    a.totals = at<uint32_t>(c->tract_out, off_to);
    a.n_reads = n;
    a.w = w; a.block = block; a.min_hits = min_hits; a.gap = gap; a.min_blocks = min_blocks; a.max_tracts = max_tracts;
    if ((rc = launch_waves(c, tps::tract_map_kernel, n, tps::TRACT_WPG, a))) return rc;
    return download(c, {{tracts, a.tracts, tr_bytes}, {found, a.found, fo_bytes}, {totals, a.totals, to_bytes}});
}

int tps_batch_end_sketch(tps_ctx* c, int32_t slot, uint64_t unit, int32_t m, int32_t k, int32_t buckets, const uint8_t* tails, const int32_t* begin,
                         const int32_t* end, int64_t n_reads, uint32_t* sketch, int64_t sketch_len, uint32_t* kept, int64_t kept_len) {
    int rc, w;
    Slot* sl;
    tps::Why why;
    if ((rc = need_batch(c, slot, &sl))) return rc;
    const int64_t n = sl->n;
    if ((rc = tps::end_sketch_check(n, unit, m, k, buckets, tails, begin, end, n_reads, sketch, sketch_len, kept, kept_len, &why))) return fail(rc, "%s", why.msg);
    if (n == 0) return TPS_OK;
    // (the pattern table, the slot's tails, its scan outputs and its plan are not touched: a scan before and after the sketch gives the same results)
    tps::Layout in, out;
    const tps::RegionAt reg = tps::region_layout(in, n);
    const size_t sk_bytes = (size_t)n * buckets * 4, kp_bytes = (size_t)n * 4;
    const size_t off_sk = out.add(sk_bytes), off_kp = out.add(kp_bytes);
    if ((rc = c->ends_in.ensure(in.total))) return rc;
    if ((rc = c->ends_out.ensure(out.total))) return rc;
    TPS_POISON(c->ends_out);
    std::vector<uint32_t> table;
    if ((rc = upload_hit_table(c, unit, m, table, &w))) return rc;
    tps::EndSketchArgs a{};
    set_batch(a, *sl);
    if ((rc = upload_region(c, c->ends_in, reg, tails, begin, end, n, a))) return rc;
    a.table = (const uint32_t*)c->tract_table.p;
    a.sketch = at<uint32_t>(c->ends_out, off_sk);
    a.kept = at<uint32_t>(c->ends_out, off_kp);
    a.n_reads = n;
    a.w = w; a.k = k; a.buckets = buckets; a.shift = 32 - tps::ends_log2(buckets);
    if ((rc = launch_waves(c, tps::end_sketch_kernel, n, tps::ENDS_WPG, a))) return rc;
    return download(c, {{sketch, a.sketch, sk_bytes}, {kept, a.kept, kp_bytes}});
}

int tps_sketch_links(tps_ctx* c, const uint32_t* sketch, int64_t n, int32_t buckets, int64_t sketch_len, int32_t min_match, int32_t max_links,
                     int32_t* degree, int64_t degree_len, int32_t* links, int64_t links_len, int32_t* matches, int64_t matches_len) {
    int rc;
    tps::Why why;
    if ((rc = bind(c))) return rc;
    if ((rc = tps::sketch_links_check(sketch, n, buckets, sketch_len, min_match, max_links, degree, degree_len, links, links_len, matches, matches_len, &why)))
        return fail(rc, "%s", why.msg);
    if (n == 0) return TPS_OK;
    std::vector<uint32_t> t((size_t)n * buckets);
    tps::links_transpose(sketch, n, buckets, t.data());
    tps::Layout out;
    const size_t t_bytes = t.size() * 4, dg_bytes = (size_t)n * 4, ln_bytes = (size_t)n * max_links * 4;
    const size_t off_dg = out.add(dg_bytes), off_ln = out.add(ln_bytes), off_ma = out.add(ln_bytes);
    if ((rc = c->links_t.ensure(t_bytes))) return rc;
    if ((rc = c->links_out.ensure(out.total))) return rc;
    TPS_POISON(c->links_out);
    HIP_TRY(hipMemcpyAsync(c->links_t.p, t.data(), t_bytes, hipMemcpyHostToDevice, c->stream));      // (pageable: the copy has left `t` when the call returns)
    tps::LinkArgs a{};
    a.t = (const uint32_t*)c->links_t.p;
    a.degree = at<int32_t>(c->links_out, off_dg);
    a.links = at<int32_t>(c->links_out, off_ln);
    a.matches = at<int32_t>(c->links_out, off_ma);
    a.n = n;
    a.buckets = buckets; a.min_match = min_match; a.max_links = max_links;
    HIP_TRY(hipMemsetAsync(a.links, 0xFF, ln_bytes, c->stream));               // -1: no link
    HIP_TRY(hipMemsetAsync(a.matches, 0, ln_bytes, c->stream));
    if ((rc = launch_waves(c, tps::sketch_links_kernel, n, tps::LINKS_WPG, a))) return rc;
    return download(c, {{degree, a.degree, dg_bytes}, {links, a.links, ln_bytes}, {matches, a.matches, ln_bytes}});
}

int tps_batch_end_window(tps_ctx* c, int32_t slot, uint64_t unit, int32_t m, int32_t k, const uint8_t* tails, const int32_t* begin, const int32_t* end,
                         int64_t n_reads, int32_t span, uint32_t* codes, int64_t codes_len, uint32_t* keep, int64_t keep_len) {
    int rc, w;
    Slot* sl;
    tps::Why why;
    if ((rc = need_batch(c, slot, &sl))) return rc;
    const int64_t n = sl->n;
    if ((rc = tps::end_window_check(n, unit, m, k, tails, begin, end, n_reads, span, codes, codes_len, keep, keep_len, &why))) return fail(rc, "%s", why.msg);
    if (n == 0) return TPS_OK;
    // (like the sketch: the pattern table, the slot's tails, its scan outputs and its plan are not touched)
    const int cdw = (span + 15) / 16, kdw = (span + 31) / 32;
    tps::Layout in, out;
    const tps::RegionAt reg = tps::region_layout(in, n);
    const size_t co_bytes = (size_t)n * cdw * 4, kp_bytes = (size_t)n * kdw * 4;
    const size_t off_co = out.add(co_bytes), off_kp = out.add(kp_bytes);
    if ((rc = c->ends_in.ensure(in.total))) return rc;
    if ((rc = c->window_out.ensure(out.total))) return rc;
    TPS_POISON(c->window_out);
    std::vector<uint32_t> table;
    if ((rc = upload_hit_table(c, unit, m, table, &w))) return rc;
    tps::EndWindowArgs a{};
    set_batch(a, *sl);
    if ((rc = upload_region(c, c->ends_in, reg, tails, begin, end, n, a))) return rc;
    a.table = (const uint32_t*)c->tract_table.p;
    a.codes = at<uint32_t>(c->window_out, off_co);
    a.keep = at<uint32_t>(c->window_out, off_kp);
    a.n_reads = n;
    a.w = w; a.k = k; a.cdw = cdw; a.kdw = kdw;
    if ((rc = launch_waves(c, tps::end_window_kernel, n, tps::ENDS_WPG, a))) return rc;
    return download(c, {{codes, a.codes, co_bytes}, {keep, a.keep, kp_bytes}});
}

int tps_window_offsets(tps_ctx* c, const uint32_t* codes, const uint32_t* keep, const int32_t* length, const int32_t* ref, int64_t n, int32_t span,
                       int32_t k, int32_t* offset, int32_t* votes, int32_t* second, int64_t out_len) {
    int rc;
    tps::Why why;
    if ((rc = bind(c))) return rc;
    if ((rc = tps::window_offsets_check(codes, keep, length, ref, n, span, k, offset, votes, second, out_len, &why))) return fail(rc, "%s", why.msg);
    if (n == 0) return TPS_OK;
    const int cdw = (span + 15) / 16, kdw = (span + 31) / 32;
    tps::Layout in, out;
    const size_t co_bytes = (size_t)n * cdw * 4, kp_bytes = (size_t)n * kdw * 4, n_bytes = (size_t)n * 4;
    const size_t in_co = in.add(co_bytes), in_kp = in.add(kp_bytes), in_len = in.add(n_bytes), in_ref = in.add(n_bytes);
    const size_t off_of = out.add(n_bytes), off_vo = out.add(n_bytes), off_se = out.add(n_bytes);
    if ((rc = c->offsets_in.ensure(in.total))) return rc;
    if ((rc = c->offsets_out.ensure(out.total))) return rc;
    TPS_POISON(c->offsets_out);
    tps::OffsetArgs a{};
    a.codes = at<const uint32_t>(c->offsets_in, in_co);
    a.keep = at<const uint32_t>(c->offsets_in, in_kp);
    a.length = at<const int32_t>(c->offsets_in, in_len);
    a.ref = at<const int32_t>(c->offsets_in, in_ref);
    HIP_TRY(hipMemcpyAsync((void*)a.codes, codes, co_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.keep, keep, kp_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.length, length, n_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.ref, ref, n_bytes, hipMemcpyHostToDevice, c->stream));
    a.offset = at<int32_t>(c->offsets_out, off_of);
    a.votes = at<int32_t>(c->offsets_out, off_vo);
    a.second = at<int32_t>(c->offsets_out, off_se);
    a.n = n;
    a.k = k; a.cdw = cdw; a.kdw = kdw;
    if ((rc = launch_waves(c, tps::window_offsets_kernel, n, tps::OFFSETS_WPG, a))) return rc;
    return download(c, {{offset, a.offset, n_bytes}, {votes, a.votes, n_bytes}, {second, a.second, n_bytes}});
}

int tps_window_place(tps_ctx* c, const uint32_t* codes, int64_t codes_len, const uint32_t* keep, int64_t keep_len, const int32_t* length, int64_t n,
                     const uint32_t* ref_codes, int64_t ref_codes_len, const uint32_t* ref_keep, int64_t ref_keep_len, const int32_t* ref_length,
                     int32_t n_ref, int32_t span, int32_t k, int32_t max_occ, int32_t* ref, int32_t* total, int32_t* runner_ref, int32_t* runner,
                     int32_t* offset, int32_t* votes, int32_t* second, int64_t out_len) {
    int rc;
    tps::Why why;
    if ((rc = bind(c))) return rc;
    const bool have_outs = ref && total && runner_ref && runner && offset && votes && second;
    if ((rc = tps::window_place_check(codes, codes_len, keep, keep_len, length, n, ref_codes, ref_codes_len, ref_keep, ref_keep_len, ref_length, n_ref, span, k,
                                      max_occ, have_outs, out_len, &why)))
        return fail(rc, "%s", why.msg);
    if (n == 0) return TPS_OK;
    const int cdw = (span + 15) / 16, kdw = (span + 31) / 32;
    tps::PlaceIndex ix;
    tps::place_index_build(ref_codes, ref_keep, ref_length, n_ref, cdw, kdw, k, max_occ, ix);
    tps::Layout in, idx;
    const size_t co_bytes = (size_t)n * cdw * 4, kp_bytes = (size_t)n * kdw * 4, n_bytes = (size_t)n * 4;
    const size_t dir_bytes = ix.dir.size() * 4, key_bytes = ix.keys.size() * 4, ent_bytes = ix.ent.size() * 4;
    const size_t in_co = in.add(co_bytes), in_kp = in.add(kp_bytes), in_len = in.add(n_bytes);
    const size_t off_dir = idx.add(dir_bytes), off_key = idx.add(key_bytes), off_ent = idx.add(ent_bytes);
    if ((rc = c->place_in.ensure(in.total))) return rc;
    if ((rc = c->place_idx.ensure(idx.total))) return rc;
    if ((rc = c->place_out.ensure(tps::PLACE_OUTS * n_bytes))) return rc;
    TPS_POISON(c->place_in);
    TPS_POISON(c->place_idx);
    TPS_POISON(c->place_out);
    tps::PlaceArgs a{};
    a.codes = at<const uint32_t>(c->place_in, in_co);
    a.keep = at<const uint32_t>(c->place_in, in_kp);
    a.length = at<const int32_t>(c->place_in, in_len);
    a.dir = at<const uint32_t>(c->place_idx, off_dir);
    a.keys = at<const uint32_t>(c->place_idx, off_key);
    a.ent = at<const uint32_t>(c->place_idx, off_ent);
    HIP_TRY(hipMemcpyAsync((void*)a.codes, codes, co_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.keep, keep, kp_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.length, length, n_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.dir, ix.dir.data(), dir_bytes, hipMemcpyHostToDevice, c->stream));
    if (key_bytes) HIP_TRY(hipMemcpyAsync((void*)a.keys, ix.keys.data(), key_bytes, hipMemcpyHostToDevice, c->stream));
    if (ent_bytes) HIP_TRY(hipMemcpyAsync((void*)a.ent, ix.ent.data(), ent_bytes, hipMemcpyHostToDevice, c->stream));
    a.out = (int32_t*)c->place_out.p;
    a.n = n;
    a.R = n_ref; a.k = k; a.cdw = cdw; a.kdw = kdw; a.shift = 32 - ix.bits;
    if ((rc = launch_waves(c, tps::window_place_kernel, n, tps::PLACE_WPG, a))) return rc;
    static_assert(tps::PLACE_OUTS == 7, "the seven outputs behind one another, n entries each");
    return download(c, {{ref, a.out, n_bytes}, {total, a.out + n, n_bytes}, {runner_ref, a.out + 2 * n, n_bytes}, {runner, a.out + 3 * n, n_bytes},
                        {offset, a.out + 4 * n, n_bytes}, {votes, a.out + 5 * n, n_bytes}, {second, a.out + 6 * n, n_bytes}});
}

int tps_window_align(tps_ctx* c, const uint32_t* codes, int64_t codes_len, const int32_t* length, int64_t n, const uint32_t* ref_codes,
                     int64_t ref_codes_len, const int32_t* ref_length, int32_t n_ref, const int32_t* ref, const int32_t* centre, int32_t span,
                     int32_t* stat, int64_t stat_len, uint16_t* cols, int64_t cols_len, const int32_t* pile_row, int32_t* pile, int32_t n_pile,
                     int64_t pile_len) {
    int rc;
    tps::Why why;
    if ((rc = bind(c))) return rc;
    if ((rc = tps::window_align_check(codes, codes_len, length, n, ref_codes, ref_codes_len, ref_length, n_ref, ref, centre, span, stat, stat_len, cols, cols_len,
                                      pile_row, pile, n_pile, pile_len, &why)))
        return fail(rc, "%s", why.msg);
    const size_t pile_bytes = pile ? (size_t)pile_len * 4 : 0;
    if (n == 0) {                                  // (no pair: an empty pile is the whole answer)
        if (pile_bytes) memset(pile, 0, pile_bytes);
        return TPS_OK;
    }
    const int cdw = (span + 15) / 16;
    tps::Layout in, out;
    const size_t co_bytes = (size_t)n * cdw * 4, rco_bytes = (size_t)n_ref * cdw * 4, n_bytes = (size_t)n * 4, nr_bytes = (size_t)n_ref * 4;
    const size_t st_bytes = (size_t)n * tps::ALIGN_STATS * 4, cl_bytes = cols ? (size_t)n * span * 2 : 0;
    const size_t in_co = in.add(co_bytes), in_rco = in.add(rco_bytes), in_len = in.add(n_bytes), in_rlen = in.add(nr_bytes), in_ref = in.add(n_bytes),
                 in_ce = in.add(n_bytes), in_pr = in.add(pile_row ? n_bytes : 0);
    const size_t off_st = out.add(st_bytes), off_cl = out.add(cl_bytes);
    if ((rc = c->align_in.ensure(in.total))) return rc;
    if ((rc = c->align_out.ensure(out.total))) return rc;
    if (pile_bytes && (rc = c->align_pile.ensure(pile_bytes))) return rc;
    TPS_POISON(c->align_out);
    if (pile_bytes) TPS_POISON(c->align_pile);
    tps::AlignArgs a{};
    a.codes = at<const uint32_t>(c->align_in, in_co);
    a.ref_codes = at<const uint32_t>(c->align_in, in_rco);
    a.length = at<const int32_t>(c->align_in, in_len);
    a.ref_length = at<const int32_t>(c->align_in, in_rlen);
    a.ref = at<const int32_t>(c->align_in, in_ref);
    a.centre = at<const int32_t>(c->align_in, in_ce);
    a.pile_row = pile_row ? at<const int32_t>(c->align_in, in_pr) : nullptr;
    HIP_TRY(hipMemcpyAsync((void*)a.codes, codes, co_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.ref_codes, ref_codes, rco_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.length, length, n_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.ref_length, ref_length, nr_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.ref, ref, n_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.centre, centre, n_bytes, hipMemcpyHostToDevice, c->stream));
    if (pile_row) HIP_TRY(hipMemcpyAsync((void*)a.pile_row, pile_row, n_bytes, hipMemcpyHostToDevice, c->stream));
    a.stat = at<int32_t>(c->align_out, off_st);
    a.cols = cols ? at<uint16_t>(c->align_out, off_cl) : nullptr;
    a.pile = pile_bytes ? (int32_t*)c->align_pile.p : nullptr;
    if (pile_bytes) HIP_TRY(hipMemsetAsync(a.pile, 0, pile_bytes, c->stream));      // (the kernel adds to it)
    a.n = n;
    a.span = span; a.cdw = cdw; a.rows = tps::align_rows(length, ref, n);
    const size_t lds_bytes = (size_t)tps::ALIGN_WPG * tps::align_lds_dw(span, cdw, a.rows) * 4;
    if (lds_bytes > c->lds_set_align) {
        HIP_TRY(hipFuncSetAttribute((const void*)tps::window_align_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        c->lds_set_align = lds_bytes;
    }
    if ((rc = launch_waves(c, tps::window_align_kernel, n, tps::ALIGN_WPG, a, lds_bytes))) return rc;
    return download(c, {{stat, a.stat, st_bytes}, {cols, a.cols, cl_bytes}, {pile, a.pile, pile_bytes}});
}

int tps_batch_adapter_find(tps_ctx* c, int32_t slot, const uint64_t* patterns, const int32_t* pat_len, int32_t n_pat, const uint8_t* tails,
                           const int32_t* begin, const int32_t* end, int64_t n_reads, uint16_t* hits, int64_t hits_len) {
    int rc;
    Slot* sl;
    tps::Why why;
    if ((rc = need_batch(c, slot, &sl))) return rc;
    const int64_t n = sl->n;
    if ((rc = tps::adapter_find_check(n, patterns, pat_len, n_pat, tails, begin, end, n_reads, hits, hits_len, &why))) return fail(rc, "%s", why.msg);
    if (n == 0) return TPS_OK;
    // (no pattern table; the slot's tails, its scan outputs and its plan are not touched: a scan before and after the call gives the same results)
    uint64_t peq[4 * tps::ADAPTER_MAX_PATTERNS];
    tps::adapter_build_peq(patterns, pat_len, n_pat, peq);
    tps::Layout in;
    const size_t peq_bytes = (size_t)n_pat * 32, len_bytes = (size_t)n_pat * 4, out_bytes = (size_t)n * n_pat * 4;
    const size_t off_peq = in.add(peq_bytes), off_len = in.add(len_bytes);
    const tps::RegionAt reg = tps::region_layout(in, n);
    if ((rc = c->adapter_in.ensure(in.total))) return rc;
    if ((rc = c->adapter_out.ensure(out_bytes))) return rc;
    TPS_POISON(c->adapter_out);
    tps::AdapterArgs a{};
    set_batch(a, *sl);
    a.peq = at<const uint64_t>(c->adapter_in, off_peq);
    a.pat_len = at<const int32_t>(c->adapter_in, off_len);
    HIP_TRY(hipMemcpyAsync((void*)a.peq, peq, peq_bytes, hipMemcpyHostToDevice, c->stream));      // (pageable: the copy has left `peq` when the call returns)
    HIP_TRY(hipMemcpyAsync((void*)a.pat_len, pat_len, len_bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = upload_region(c, c->adapter_in, reg, tails, begin, end, n, a))) return rc;
    a.hits = (uint32_t*)c->adapter_out.p;
    a.n_reads = n;
    a.n_pat = n_pat;
    if ((rc = launch_waves(c, tps::adapter_find_kernel, n, tps::ADAPTER_WPG, a))) return rc;
    return download(c, {{hits, a.hits, out_bytes}});
}

int tps_batch_boundary_refine(tps_ctx* c, int32_t slot, uint64_t unit, int32_t m, const uint8_t* tails, const int32_t* begin, const int32_t* end,
                              const int32_t* at_in, int64_t n_reads, int32_t hit, int32_t miss, int32_t sep, tps_refine* out, int64_t out_len) {
    int rc, w;
    Slot* sl;
    tps::Why why;
    if ((rc = need_batch(c, slot, &sl))) return rc;
    const int64_t n = sl->n;
    if ((rc = tps::boundary_refine_check(n, sl->h_offsets.data(), unit, m, tails, begin, end, at_in, n_reads, hit, miss, sep, out, out_len, &why)))
        return fail(rc, "%s", why.msg);
    if (n == 0) return TPS_OK;
    // (the pattern table, the slot's tails, its scan outputs and its plan are not touched: a scan before and after the call gives the same results)
    tps::Layout in;
    const tps::RegionAt reg = tps::region_layout(in, n);
    const size_t off_at = in.add((size_t)n * 4), out_bytes = (size_t)n * sizeof(tps_refine);
    if ((rc = c->refine_in.ensure(in.total))) return rc;
    if ((rc = c->refine_out.ensure(out_bytes))) return rc;
    TPS_POISON(c->refine_out);
    std::vector<uint32_t> table;
    if ((rc = upload_hit_table(c, unit, m, table, &w))) return rc;
    tps::RefineArgs a{};
    set_batch(a, *sl);
    if ((rc = upload_region(c, c->refine_in, reg, tails, begin, end, n, a))) return rc;
    a.at = at<const int32_t>(c->refine_in, off_at);
    HIP_TRY(hipMemcpyAsync((void*)a.at, at_in, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    a.table = (const uint32_t*)c->tract_table.p;
    a.out = (tps_refine*)c->refine_out.p;
    a.n_reads = n;
    a.w = w; a.hit = hit; a.miss = miss; a.sep = sep;
    a.bal_dw = tps::refine_ballot_dw(n, sl->h_offsets.data(), begin, end, w);
    const size_t lds_bytes = (size_t)(tps::TRACT_TABLE_DW + tps::REFINE_WPG * tps::refine_lds_dw(a.bal_dw)) * 4;
    if (lds_bytes > c->lds_set_refine) {
        HIP_TRY(hipFuncSetAttribute((const void*)tps::boundary_refine_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        c->lds_set_refine = lds_bytes;
    }
    if ((rc = launch_waves(c, tps::boundary_refine_kernel, n, tps::REFINE_WPG, a, lds_bytes))) return rc;
    return download(c, {{out, a.out, out_bytes}});
}

int tps_batch_mod_profile(tps_ctx* c, int32_t slot, const uint8_t* tails, const int32_t* begin, const int32_t* end, const int32_t* origin, int64_t n_reads,
                          const int64_t* mod_off, const uint32_t* delta, const uint8_t* prob, int64_t n_mods, int32_t w, int32_t nb0, int32_t nb1, int32_t hi,
                          int32_t lo, tps_mod_row* rows, int64_t rows_len, tps_mod_bin* bins, int64_t bins_len) {
    int rc;
    Slot* sl;
    tps::Why why;
    if ((rc = need_batch(c, slot, &sl))) return rc;
    const int64_t n = sl->n;
    if ((rc = tps::mod_profile_check(n, sl->h_offsets.data(), tails, begin, end, origin, n_reads, mod_off, delta, prob, n_mods, w, nb0, nb1, hi, lo, rows, rows_len,
                                     bins, bins_len, &why)))
        return fail(rc, "%s", why.msg);
    if (n == 0) return TPS_OK;
    // (no pattern table; the slot's tails, its scan outputs and its plan are not touched: a scan before and after the call gives the same results)
    tps::Layout in, out;
    const tps::RegionAt reg = tps::region_layout(in, n);
    const size_t off_origin = in.add((size_t)n * 4), off_mo = in.add((size_t)(n + 1) * 8, 8), off_delta = in.add((size_t)n_mods * 4), off_prob = in.add((size_t)n_mods);
    const size_t row_bytes = (size_t)n * sizeof(tps_mod_row), bin_bytes = (size_t)n * (nb0 + nb1) * sizeof(tps_mod_bin);
    const size_t off_rows = out.add(row_bytes, 16), off_bins = out.add(bin_bytes, 16);
    if ((rc = c->mod_in.ensure(in.total))) return rc;
    if ((rc = c->mod_out.ensure(out.total))) return rc;
    TPS_POISON(c->mod_out);
    tps::ModArgs a{};
    set_batch(a, *sl);
    if ((rc = upload_region(c, c->mod_in, reg, tails, begin, end, n, a))) return rc;
    a.origin = at<const int32_t>(c->mod_in, off_origin);
    a.mod_off = at<const int64_t>(c->mod_in, off_mo);
    a.delta = at<const uint32_t>(c->mod_in, off_delta);
    a.prob = at<const uint8_t>(c->mod_in, off_prob);
    HIP_TRY(hipMemcpyAsync((void*)a.origin, origin, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void*)a.mod_off, mod_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n_mods > 0) {
        HIP_TRY(hipMemcpyAsync((void*)a.delta, delta, (size_t)n_mods * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync((void*)a.prob, prob, (size_t)n_mods, hipMemcpyHostToDevice, c->stream));
    }
    a.rows = at<tps_mod_row>(c->mod_out, off_rows);
    a.bins = at<tps_mod_bin>(c->mod_out, off_bins);
    a.n_reads = n;
    a.w = w; a.nb0 = nb0; a.nb1 = nb1; a.hi = hi; a.lo = lo;
    if ((rc = launch_waves(c, tps::mod_profile_kernel, n, tps::MOD_WPG, a))) return rc;
    return download(c, {{rows, a.rows, row_bytes}, {bins, a.bins, bin_bytes}});
}

int tps_batch_set_tails(tps_ctx* c, int32_t slot, const uint8_t* tails) {
    int rc;
    if ((rc = bind(c))) return rc;
    Slot* sl = get_slot(c, slot);
    if (!sl) return TPS_E_ARG;
    if (sl->n < 0) return fail(TPS_E_STATE, "no batch uploaded in this slot");
    if (!tails && sl->n > 0) return fail(TPS_E_ARG, "null tails");
    if ((rc = sl->tails.ensure((size_t)std::max<int64_t>(sl->n, 1)))) return rc;
    if (sl->n) HIP_TRY(hipMemcpyAsync(sl->tails.p, tails, (size_t)sl->n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    sl->has_tails = true;
    return TPS_OK;
}

int tps_batch_scan(tps_ctx* c, int32_t slot, const tps_params* prm) {
    int rc;
    if ((rc = bind(c))) return rc;
    Slot* sl = get_slot(c, slot);
    if (!sl) return TPS_E_ARG;
    if (!prm) return fail(TPS_E_ARG, "null params");
    return do_scan(c, *sl, *prm);
}

int tps_sync(tps_ctx* c) {
    int rc;
    if ((rc = bind(c))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return TPS_OK;
}

static int need_scanned(tps_ctx* c, int slot, Slot** out) {
    int rc;
    if ((rc = bind(c))) return rc;
    Slot* sl = (slot == INTERNAL_SLOT) ? &c->slots[INTERNAL_SLOT] : get_slot(c, slot);
    if (!sl) return TPS_E_ARG;
    if (!sl->scanned) return fail(TPS_E_STATE, "slot has not been scanned");
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = sl;
    return TPS_OK;
}

int tps_batch_results(tps_ctx* c, int32_t slot, tps_read_result* out, int64_t n) {
    Slot* sl;
    int rc;
    if ((rc = need_scanned(c, slot, &sl))) return rc;
    if (n != sl->n || (n > 0 && !out)) return fail(TPS_E_ARG, "result buffer must hold %lld reads", (long long)sl->n);
    if (n) memcpy(out, sl->h_results, (size_t)n * sizeof(tps_read_result));
    return TPS_OK;
}

int tps_batch_window_offsets(tps_ctx* c, int32_t slot, int64_t* win_off, int64_t n1) {
    Slot* sl;
    int rc;
    if ((rc = need_scanned(c, slot, &sl))) return rc;
    if (n1 != sl->n + 1 || !win_off) return fail(TPS_E_ARG, "win_off must hold n+1 entries");
    memcpy(win_off, sl->lay.win_off.data(), (size_t)n1 * 8);
    return TPS_OK;
}

int tps_batch_window_sums(tps_ctx* c, int32_t slot, int32_t* sums, int64_t nw) {
    Slot* sl;
    int rc;
    if ((rc = need_scanned(c, slot, &sl))) return rc;
    if (!(sl->last_flags & TPS_F_STORE_SUMS)) return fail(TPS_E_STATE, "last scan did not store window sums");
    if (nw != sl->lay.win_off[(size_t)sl->n] || (nw > 0 && !sums)) return fail(TPS_E_ARG, "sums must hold %lld windows", (long long)sl->lay.win_off[(size_t)sl->n]);
    if (nw && sl->args.variant) {
        // fused kernels: 16-bit sums in the padded device layout -> the caller's contiguous int32 array
        const int64_t n16 = sl->lay.win_off16[(size_t)sl->n];
        sl->h_sums16.resize((size_t)n16);
        HIP_TRY(hipMemcpy(sl->h_sums16.data(), sl->sums.p, (size_t)n16 * 2, hipMemcpyDeviceToHost));
        tps::widen_sums16(sl->h_sums16.data(), sl->lay.win_off16.data(), sl->lay.win_off.data(), 0, sl->n, sums);
    } else if (nw) {
        HIP_TRY(hipMemcpy(sums, sl->sums.p, (size_t)nw * 4, hipMemcpyDeviceToHost));
    }
    // (no kernel wrote the windows of the reads that do not pass: they are handed out as zeros)
    tps::clear_skipped_windows(sl->h_results, sl->lay.win_off.data(), sl->n, 1, 4, 0, nw, sums);
    return TPS_OK;
}

int tps_batch_read_sums(tps_ctx* c, int32_t slot, int64_t read, int32_t* sums, int64_t nw) {
    Slot* sl;
    int rc;
    if ((rc = need_scanned(c, slot, &sl))) return rc;
    if (!(sl->last_flags & TPS_F_WINDOWS)) return fail(TPS_E_STATE, "last scan did not run the window step");
    if (read < 0 || read >= sl->n) return fail(TPS_E_ARG, "read %lld out of range", (long long)read);
    const int64_t lo = sl->lay.win_off[(size_t)read], cnt = sl->lay.win_off[(size_t)read + 1] - lo;
    if (nw != cnt || (nw > 0 && !sums)) return fail(TPS_E_ARG, "sums must hold %lld windows", (long long)cnt);
    if (!nw) return TPS_OK;
    if (sl->args.variant) {
        sl->h_sums16.resize((size_t)nw);
        HIP_TRY(hipMemcpy(sl->h_sums16.data(), (const uint16_t*)sl->sums.p + sl->lay.win_off16[(size_t)read], (size_t)nw * 2, hipMemcpyDeviceToHost));
        for (int64_t w = 0; w < nw; ++w) sums[w] = (int32_t)sl->h_sums16[(size_t)w];
    } else {
        HIP_TRY(hipMemcpy(sums, (const int32_t*)sl->sums.p + lo, (size_t)nw * 4, hipMemcpyDeviceToHost));
    }
    tps::clear_skipped_windows(sl->h_results, sl->lay.win_off.data(), sl->n, 1, 4, lo, lo + nw, sums);
    return TPS_OK;
}

int tps_batch_window_raw(tps_ctx* c, int32_t slot, uint8_t* raw, int64_t nwp) {
    Slot* sl;
    int rc;
    if ((rc = need_scanned(c, slot, &sl))) return rc;
    if (!(sl->last_flags & TPS_F_STORE_RAW)) return fail(TPS_E_STATE, "last scan did not store raw counts");
    int64_t want = sl->lay.win_off[(size_t)sl->n] * sl->plan_p;
    if (nwp != want || (nwp > 0 && !raw)) return fail(TPS_E_ARG, "raw must hold %lld bytes", (long long)want);
    if (nwp) HIP_TRY(hipMemcpy(raw, sl->raw.p, (size_t)nwp, hipMemcpyDeviceToHost));
    tps::clear_skipped_windows(sl->h_results, sl->lay.win_off.data(), sl->n, sl->plan_p, 1, 0, nwp, raw);
    return TPS_OK;
}

// Raw rows of selected reads -> a file, without a stop in the caller's memory (include/topsicle_hip.h).  The selected reads' rows
// are runs of the slot's raw buffer; runs closer than RAW_GAP are fetched as one stretch (what lies between is copied and skipped:
// cheaper than a copy call per read), stretches are cut into pieces of RAW_STAGE bytes, piece j + 1 is copied into one pinned
// buffer while piece j is written from the other (pwritev of the wanted parts only) and checksummed.
constexpr size_t RAW_STAGE = (size_t)32 << 20;
constexpr int64_t RAW_GAP = 256 << 10;

int tps_batch_raw_to_fd(tps_ctx* c, int32_t slot, const int64_t* reads, int64_t n_sel, int fd, int64_t file_off,
                        tps_crc32_fn crc_fn, uint32_t* crc_out, int64_t* bytes_out) {
    Slot* sl;
    int rc;
    if ((rc = need_scanned(c, slot, &sl))) return rc;
    if (!(sl->last_flags & TPS_F_STORE_RAW)) return fail(TPS_E_STATE, "last scan did not store raw counts");
    if (n_sel < 0 || (n_sel > 0 && !reads) || fd < 0 || file_off < 0) return fail(TPS_E_ARG, "bad arguments");
    if (crc_out) *crc_out = 0;
    if (bytes_out) *bytes_out = 0;
    const int64_t P = sl->plan_p;
    struct Run { int64_t lo, hi; };                    // bytes of the raw buffer
    std::vector<Run> runs;
    int64_t prev = -1;
    for (int64_t j = 0; j < n_sel; ++j) {
        const int64_t i = reads[j];
        if (i <= prev || i >= sl->n) return fail(TPS_E_ARG, "reads[] must be ascending indices of the batch (entry %lld)", (long long)j);
        prev = i;
        const int64_t lo = sl->lay.win_off[(size_t)i] * P, hi = sl->lay.win_off[(size_t)i + 1] * P;
        if (hi == lo) continue;
        if (!runs.empty() && runs.back().hi == lo) runs.back().hi = hi;
        else runs.push_back({lo, hi});
    }
    if (runs.empty()) return TPS_OK;
    for (int i = 0; i < 2; ++i) {
        if (!c->raw_stage[i]) HIP_TRY(hipHostMalloc(&c->raw_stage[i], RAW_STAGE, hipHostMallocPortable));
        if (!c->raw_ev[i]) HIP_TRY(hipEventCreateWithFlags(&c->raw_ev[i], hipEventDisableTiming));
    }
    // pieces: [first run, last run) + the device span [lo, hi) that covers them (hi - lo <= RAW_STAGE); a run longer than what is
    // left of a piece is split
    struct Piece { size_t r0, r1; int64_t lo, hi; };
    std::vector<Piece> pieces;
    {
        std::vector<Run> cut;                          // runs split at piece boundaries, in order
        size_t i = 0;
        int64_t pos = runs[0].lo;
        while (i < runs.size()) {
            Piece pc{cut.size(), cut.size(), pos, pos};
            while (i < runs.size()) {
                const int64_t start = std::max(pos, runs[i].lo);
                if (pc.r1 > pc.r0 && (start - pc.hi > RAW_GAP || start >= pc.lo + (int64_t)RAW_STAGE)) break;
                if (pc.r1 == pc.r0) pc.lo = start;
                const int64_t end = std::min(runs[i].hi, pc.lo + (int64_t)RAW_STAGE);
                if (end <= start) break;
                cut.push_back({start, end});
                pc.r1 = cut.size();
                pc.hi = end;
                pos = end;
                if (end == runs[i].hi) { ++i; if (i < runs.size()) pos = runs[i].lo; }
                else break;                            // the piece is full
            }
            pieces.push_back(pc);
        }
        runs.swap(cut);
    }
    auto enqueue = [&](size_t j) -> int {
        const Piece& pc = pieces[j];
        HIP_TRY(hipMemcpyAsync(c->raw_stage[j & 1], (const uint8_t*)sl->raw.p + pc.lo, (size_t)(pc.hi - pc.lo), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(c->raw_ev[j & 1], c->stream));
        return TPS_OK;
    };
    if ((rc = enqueue(0))) return rc;
    uint32_t crc = 0;
    int64_t written = 0;
    std::vector<struct iovec> iov;
    for (size_t j = 0; j < pieces.size(); ++j) {
        if (j + 1 < pieces.size() && (rc = enqueue(j + 1))) { (void)hipStreamSynchronize(c->stream); return rc; }
        HIP_TRY(hipEventSynchronize(c->raw_ev[j & 1]));
        const Piece& pc = pieces[j];
        const uint8_t* base = (const uint8_t*)c->raw_stage[j & 1];
        // (zero rows for the reads that do not pass, before the piece is checksummed and written)
        tps::clear_skipped_windows(sl->h_results, sl->lay.win_off.data(), sl->n, P, 1, pc.lo, pc.hi, c->raw_stage[j & 1]);
        iov.clear();
        for (size_t r = pc.r0; r < pc.r1; ++r) {
            const uint8_t* p = base + (runs[r].lo - pc.lo);
            const size_t len = (size_t)(runs[r].hi - runs[r].lo);
            if (crc_fn) crc = crc_fn(crc, p, (int64_t)len);
            iov.push_back({(void*)p, len});
        }
        size_t first = 0;
        while (first < iov.size()) {
            const int cnt = (int)std::min<size_t>(iov.size() - first, 1024);
            const ssize_t w = pwritev(fd, iov.data() + first, cnt, (off_t)(file_off + written));
            if (w < 0) {
                if (errno == EINTR) continue;
                const int e = errno;
                (void)hipStreamSynchronize(c->stream);
                return fail(TPS_E_ARG, "pwritev: %s", strerror(e));
            }
            written += w;
            size_t left = (size_t)w;
            while (first < iov.size() && left >= iov[first].iov_len) { left -= iov[first].iov_len; ++first; }
            if (left) { iov[first].iov_base = (char*)iov[first].iov_base + left; iov[first].iov_len -= left; }
        }
    }
    if (crc_out) *crc_out = crc;
    if (bytes_out) *bytes_out = written;
    return TPS_OK;
}

int tps_batch_trc_counts(tps_ctx* c, int32_t slot, int32_t* c_start, int32_t* c_end, int64_t n) {
    Slot* sl;
    int rc;
    if ((rc = need_scanned(c, slot, &sl))) return rc;
    if (!(sl->last_flags & TPS_F_STEP1)) return fail(TPS_E_STATE, "last scan did not run step 1");
    if (n != sl->n || (n > 0 && (!c_start || !c_end))) return fail(TPS_E_ARG, "count buffers must hold n*P entries");
    size_t bytes = (size_t)n * (size_t)sl->plan_p * 4;
    if (bytes) {
        HIP_TRY(hipMemcpy(c_start, sl->c_start.p, bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c_end, sl->c_end.p, bytes, hipMemcpyDeviceToHost));
    }
    return TPS_OK;
}

int64_t tps_window_count(int64_t L, int32_t W, int32_t s, int32_t t, int32_t M) { return window_count(L, W, s, t, M); }

int tps_trc_counts(tps_ctx* c, const uint8_t* bases, const int64_t* offsets, int64_t n, int32_t no_bp,
                   int32_t* c_start, int32_t* c_end) {
    int rc;
    if ((rc = bind(c))) return rc;
    Slot& sl = c->slots[INTERNAL_SLOT];
    if ((rc = do_upload(c, sl, bases, offsets, n))) return rc;
    tps_params p{};
    p.no_bp = no_bp; p.min_len = 0; p.min_count = 0; p.window = 100; p.slide = 6; p.trimfirst = 0; p.maxlen = 0;
    p.jump = 5; p.min_size = 2; p.flags = TPS_F_STEP1;
    if ((rc = do_scan(c, sl, p))) return rc;
    return tps_batch_trc_counts(c, INTERNAL_SLOT, c_start, c_end, n);
}

int tps_window_counts(tps_ctx* c, const uint8_t* bases, const int64_t* offsets, const uint8_t* tails, int64_t n,
                      int32_t W, int32_t s, int32_t t, int32_t M, const int64_t* win_off, int32_t* sums, uint8_t* raw) {
    int rc;
    if ((rc = bind(c))) return rc;
    if (!win_off || (n > 0 && !tails)) return fail(TPS_E_ARG, "null win_off / tails");
    Slot& sl = c->slots[INTERNAL_SLOT];
    if ((rc = do_upload(c, sl, bases, offsets, n))) return rc;
    if ((rc = sl.tails.ensure((size_t)std::max<int64_t>(n, 1)))) return rc;
    if (n) HIP_TRY(hipMemcpy(sl.tails.p, tails, (size_t)n, hipMemcpyHostToDevice));
    sl.has_tails = true;
    tps_params p{};
    p.no_bp = 0; p.window = W; p.slide = s; p.trimfirst = t; p.maxlen = M; p.jump = 5; p.min_size = 2;
    p.flags = TPS_F_WINDOWS | TPS_F_TAILS_IN | TPS_F_STORE_SUMS | (raw ? TPS_F_STORE_RAW : 0u);
    if ((rc = do_scan(c, sl, p))) return rc;
    for (int64_t i = 0; i <= n; ++i)
        if (win_off[i] != sl.lay.win_off[(size_t)i])
            return fail(TPS_E_ARG, "win_off[%lld]=%lld does not match the window layout (%lld)", (long long)i,
                        (long long)win_off[i], (long long)sl.lay.win_off[(size_t)i]);
    int64_t nw = sl.lay.win_off[(size_t)n];
    if ((rc = tps_batch_window_sums(c, INTERNAL_SLOT, sums, nw))) return rc;
    if (raw && (rc = tps_batch_window_raw(c, INTERNAL_SLOT, raw, nw * c->pat.P))) return rc;
    return TPS_OK;
}

int tps_binseg_l2_ties(tps_ctx* c, const int32_t* sums, const int64_t* win_off, int64_t n, int32_t n_patterns,
                       int32_t jump, int32_t min_size, int32_t* bkp, double* gain, uint8_t* tie);
int tps_binseg_l2(tps_ctx* c, const int32_t* sums, const int64_t* win_off, int64_t n, int32_t n_patterns,
                  int32_t jump, int32_t min_size, int32_t* bkp, double* gain) {
    return tps_binseg_l2_ties(c, sums, win_off, n, n_patterns, jump, min_size, bkp, gain, nullptr);
}

int tps_binseg_l2_ties(tps_ctx* c, const int32_t* sums, const int64_t* win_off, int64_t n, int32_t n_patterns,
                       int32_t jump, int32_t min_size, int32_t* bkp, double* gain, uint8_t* tie) {
    int rc;
    if ((rc = bind(c))) return rc;
    if (n < 0 || !win_off || !bkp || jump < 1 || min_size < 1 || n_patterns < 1) return fail(TPS_E_ARG, "bad arguments");
    if (n == 0) return TPS_OK;
    const int64_t nw = win_off[n];
    if (nw > 0 && !sums) return fail(TPS_E_ARG, "null sums");
    for (int64_t i = 0; i < n; ++i) {
        // the kernel adds a read's sums up in 32 bits and compares d^2 * den in 128 bits (d <= len * total, den <= len^2 / 4)
        const int64_t lo = win_off[i], len = win_off[i + 1] - lo;
        if (len < 0 || lo < 0 || lo + len > nw) return fail(TPS_E_ARG, "win_off not monotone at %lld", (long long)i);
        if (len > 500000) return fail(TPS_E_CAPACITY, "read %lld has %lld windows (max 500000)", (long long)i, (long long)len);
        uint64_t tot = 0;
        for (int64_t w = 0; w < len; ++w) {
            if (sums[lo + w] < 0) return fail(TPS_E_ARG, "negative window sum at read %lld", (long long)i);
            tot += (uint64_t)sums[lo + w];
        }
        if (tot >> 32 || (double)len * (double)len * (double)tot >= 18446744073709551616.0)
            return fail(TPS_E_CAPACITY, "window sums of read %lld exceed the change-point arithmetic (total %llu over %lld windows)",
                        (long long)i, (unsigned long long)tot, (long long)len);
    }
    Slot& sl = c->slots[INTERNAL_SLOT];
    if ((rc = sl.sums.ensure((size_t)std::max<int64_t>(nw, 1) * 4))) return rc;
    if ((rc = sl.win_off.ensure((size_t)(n + 1) * 8))) return rc;
    if ((rc = sl.results.ensure((size_t)n * 17))) return rc;          // gain (8n), bkp (4n), tie (n): gain first for alignment
    TPS_POISON(sl.results);
    sl.planned = false;                                                // the slot's plan buffers were overwritten
    sl.wplanned = false;
    sl.scanned = false;
    if (nw) HIP_TRY(hipMemcpyAsync(sl.sums.p, sums, (size_t)nw * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(sl.win_off.p, win_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    tps::BinsegArgs a{};
    a.sums = (const int32_t*)sl.sums.p;
    a.win_off = (const int64_t*)sl.win_off.p;
    a.gain = (double*)sl.results.p;
    a.bkp = (int32_t*)((char*)sl.results.p + (size_t)n * 8);
    a.tie = (uint8_t*)sl.results.p + (size_t)n * 12;
    a.n_reads = n;
    a.n_patterns = n_patterns;
    a.jump = jump;
    a.min_size = min_size;
    hipLaunchKernelGGL(tps_binseg_kernel, dim3((unsigned)((n + tps::WPG - 1) / tps::WPG)), dim3(tps::NT * tps::WPG), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(bkp, a.bkp, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (gain) HIP_TRY(hipMemcpyAsync(gain, a.gain, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    if (tie) HIP_TRY(hipMemcpyAsync(tie, a.tie, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return TPS_OK;
}

int tps_kernel_time_ms(tps_ctx* c, int32_t* n_launches, double* total_ms, double* mean_ms) {
    int rc;
    if ((rc = bind(c))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    double tot = 0.0;
    for (size_t i = c->ev_base; i < c->ev_used; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_pool[i].a, c->ev_pool[i].b));
        tot += ms;
    }
    const size_t cnt = c->ev_used - c->ev_base;
    if (n_launches) *n_launches = (int32_t)cnt;
    if (total_ms) *total_ms = tot;
    if (mean_ms) *mean_ms = cnt ? tot / (double)cnt : 0.0;
    return TPS_OK;
}

int tps_ctx_debug_option(tps_ctx* c, const char* key, int64_t value) {
    if (!c || !key) return fail(TPS_E_ARG, "null argument");
    const std::string k(key);
    if (k == "event_stride") c->event_stride = (int)std::max<int64_t>(1, value);
    else if (k == "no_events") c->no_events = value != 0;
    else if (k == "force_generic") c->knobs.force_generic = value != 0;
    else if (k == "spans_per_tile") c->knobs.spans_per_tile = (int)std::max<int64_t>(0, value);
    else if (k == "force_pair") c->knobs.force_pair = value != 0;
    else if (k == "so_order") c->knobs.so_order = (int)value;
    else if (k == "wpg") c->knobs.wpg = (int)value;
    else if (k == "lc_lds") c->knobs.lc_lds = value != 0;       // 0: the default kernels' candidate sums off-chip, as every other kernel's (A/B, tests)
    else if (k == "stamps") c->want_stamps = value != 0;
    else if (k == "file_order") c->file_order = value != 0;
    else if (k == "no_stride") c->no_stride = value != 0;
    else if (k == "no_inline_rows") c->no_inline_rows = value != 0;
    else if (k == "poison") {
        if (value < 0 || value > 255) return fail(TPS_E_ARG, "poison must be 0 (off) or a fill byte 1..255");
        c->poison = (int)value;
    }
    else return fail(TPS_E_ARG, "unknown debug option '%s' (event_stride, no_events, force_generic, spans_per_tile, force_pair, so_order, wpg, lc_lds, stamps, file_order, no_stride, no_inline_rows, poison)", key);
    drop_plans(c);
    return TPS_OK;
}

/* per-read phase clock stamps of the last scan (only a -DTPS_STAMPS build of the kernels writes them; option "stamps") */
int tps_debug_stamps_get(tps_ctx* c, int32_t slot, uint64_t* out, int64_t n) {
    Slot* sl;
    int rc;
    if ((rc = need_scanned(c, slot, &sl))) return rc;
    if (!sl->stamps.p || n != sl->n) return fail(TPS_E_STATE, "no stamps recorded");
    HIP_TRY(hipMemcpy(out, sl->stamps.p, (size_t)n * 16 * 8, hipMemcpyDeviceToHost));
    return TPS_OK;
}

int tps_kernel_time_reset(tps_ctx* c) {
    int rc;
    if ((rc = bind(c))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ev_base = c->ev_used;
    c->launch_seq = 0;                             // the next launch is a timed one
    return TPS_OK;
}

}  // extern "C"
