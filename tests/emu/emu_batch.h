// TEST INFRASTRUCTURE ONLY -- what every host emulation (emu_*.cpp) sets up before it runs a kernel's text: the packed batch and one
// wave's LDS slice.  Never linked into the product.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../topsicle_amd/csrc/tps_pack.h"

namespace emu {

// The packed batch, exactly as the library keeps it in HBM (tps_pack.h: the library's own packer).  Words the layout does not own
// are filled with garbage: a kernel must never let them count.  base_shift moves the batch inside its buffer by whole quads (the
// device only ever sees 16-byte aligned quads).
struct Batch {
    std::vector<tps_read_desc> desc;
    std::vector<uint32_t> seq2;
    std::vector<uint16_t> inv;
    Batch(const uint8_t* bases, const int64_t* offsets, int64_t n, int base_shift = 0) : desc((size_t)(n > 0 ? n : 1)) {
        const int64_t n_words = tps::pack_layout(offsets, n, desc.data());
        const int64_t lead = 4 * (int64_t)(base_shift & 3);
        seq2.assign((size_t)(n_words + lead + 8), 0xDEADBEEFu);
        inv.assign((size_t)(n_words + lead + 8), (uint16_t)0xFFFFu);
        for (int64_t i = 0; i < n; ++i) desc[(size_t)i].word_off += lead;
        tps::pack_range(bases, offsets, 0, n, desc.data(), seq2.data(), inv.data());
    }
    // ... in a kernel's arguments
    template <class A>
    void set(A& a) const {
        a.seq2 = seq2.data();
        a.inv = inv.data();
        a.desc = desc.data();
    }
};

// Exactly one wave's slice of `dw` dwords, 16-byte aligned like LDS: a sanitizer build sees every access past it.  poisoned(): the
// slice before a read (or row) -- LDS content is undefined at workgroup start.
struct WaveLds {
    uint32_t* p = nullptr;
    int dw;
    explicit WaveLds(int dw_) : dw(dw_) {
        if (posix_memalign((void**)&p, 16, (size_t)dw * 4)) abort();
    }
    WaveLds(const WaveLds&) = delete;
    WaveLds& operator=(const WaveLds&) = delete;
    ~WaveLds() { free(p); }
    uint32_t* poisoned() {
        for (int i = 0; i < dw; ++i) p[i] = 0xDEADBEEFu;
        return p;
    }
};

}  // namespace emu
