// tps_layout.h -- pieces behind one another in one buffer: the read-analysis calls (topsicle_hip.hip) lay out every staging and output
// buffer with it, once, and take the allocation's size, the kernel's pointers and the downloads from the offsets it handed out.
// Host code without HIP (tests/emu/layout_main.cpp checks it against the formulas written out by hand).
#pragma once
#include <cstddef>
#include <cstdint>

namespace tps {

struct Layout {
    size_t total = 0;            // bytes up to the end of the last piece: what the buffer has to hold
    // the offset of a piece of `bytes` bytes that starts on a multiple of `align` (a power of two)
    size_t add(size_t bytes, size_t align = 4) {
        const size_t off = (total + align - 1) & ~(align - 1);
        total = off + bytes;
        return off;
    }
};

// tails / begin / end of n reads, as the variant census, the end sketch, the end window and the adapter call stage them: the bytes
// and the first of the two int32 arrays on 16-byte boundaries
struct RegionAt { size_t tails, begin, end; };
inline RegionAt region_layout(Layout& l, int64_t n) {
    RegionAt at;
    at.tails = l.add((size_t)n, 16);
    at.begin = l.add((size_t)n * 4, 16);
    at.end = l.add((size_t)n * 4);
    return at;
}

}  // namespace tps
