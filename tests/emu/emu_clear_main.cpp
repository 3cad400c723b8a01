// TEST INFRASTRUCTURE ONLY -- stand-alone program for the sanitizers (its own main, nothing loaded into Python):
//   g++ -fsanitize=address,undefined emu_clear_main.cpp && ./a.out
// The host rule behind "reads that do not pass come down as zeros" (include/topsicle_hip.h): tps::clear_skipped_windows and
// tps::widen_sums16 of csrc/tps_plan.h, the very functions the library's downloads and the emulation call.  Every buffer is allocated
// at exactly its size (one element past it is an AddressSanitizer error), filled with garbage, cleared as a whole and piece by piece
// -- every pair of cuts, so pieces begin and end inside reads as tps_batch_raw_to_fd's do -- and compared with a restatement of the
// rule that walks the reads one element at a time.
#define TPS_EMU 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../topsicle_amd/csrc/tps_plan.h"

static int g_checks = 0;

#define REQUIRE(cond, ...)                                                       \
    do {                                                                         \
        if (!(cond)) {                                                           \
            printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);             \
            printf(__VA_ARGS__);                                                 \
            printf("\n");                                                        \
            exit(1);                                                             \
        }                                                                        \
        ++g_checks;                                                              \
    } while (0)

struct Batch {
    const char* name;
    std::vector<int64_t> nwin;     // windows per read
    std::vector<int> pass;
};

static uint8_t garbage(int64_t i) { return (uint8_t)(0xEE ^ (i * 37)) | 1u; }      // (never zero)

// elements [lo, hi) of a per-window output (read i owns [win_off[i] * scale, win_off[i + 1] * scale), `unit` bytes per element):
// garbage, cleared by the function under test, against the rule stated element by element
static void check_piece(const Batch& b, const std::vector<tps_read_result>& res, const std::vector<int64_t>& win_off, int64_t scale, size_t unit,
                        int64_t lo, int64_t hi) {
    const int64_t n = (int64_t)b.nwin.size();
    std::vector<uint8_t> buf((size_t)(hi - lo) * unit);
    for (size_t i = 0; i < buf.size(); ++i) buf[i] = garbage((int64_t)i + lo);
    const int64_t cleared = tps::clear_skipped_windows(res.data(), win_off.data(), n, scale, unit, lo, hi, buf.empty() ? nullptr : buf.data());
    int64_t want_cleared = 0;
    for (int64_t r = 0; r < n; ++r)
        for (int64_t e = win_off[(size_t)r] * scale; e < win_off[(size_t)r + 1] * scale; ++e) {
            if (e < lo || e >= hi) continue;
            for (size_t by = 0; by < unit; ++by) {
                const size_t at = (size_t)(e - lo) * unit + by;
                const uint8_t want = b.pass[(size_t)r] ? garbage((int64_t)at + lo) : 0;
                REQUIRE(buf[at] == want, "%s scale %lld unit %zu piece [%lld, %lld): read %lld element %lld byte %zu is %u, want %u", b.name,
                        (long long)scale, unit, (long long)lo, (long long)hi, (long long)r, (long long)e, by, buf[at], want);
            }
            want_cleared += !b.pass[(size_t)r];
        }
    REQUIRE(cleared == want_cleared, "%s: cleared %lld elements, want %lld", b.name, (long long)cleared, (long long)want_cleared);
}

static void run(const Batch& b) {
    const int64_t n = (int64_t)b.nwin.size();
    std::vector<int64_t> win_off((size_t)n + 1, 0), win_off16((size_t)n + 1, 0);
    std::vector<tps_read_result> res((size_t)n);
    memset(res.data(), 0xEE, res.size() * sizeof(tps_read_result));
    for (int64_t i = 0; i < n; ++i) {
        win_off[(size_t)i + 1] = win_off[(size_t)i] + b.nwin[(size_t)i];
        win_off16[(size_t)i + 1] = win_off16[(size_t)i] + tps::sums16_slots(b.nwin[(size_t)i]);
        res[(size_t)i].pass = b.pass[(size_t)i];
    }
    const int64_t nw = win_off[(size_t)n];
    // S_w (int32) and raw rows (P = 1, 4, 7 bytes per window): the whole array, every piece [lo, hi) of it, one read at a time
    for (int P : {0, 1, 4, 7}) {
        const int64_t scale = P ? P : 1;
        const size_t unit = P ? 1 : 4;
        const int64_t tot = nw * scale;
        check_piece(b, res, win_off, scale, unit, 0, tot);
        const int64_t step = tot > 96 ? tot / 48 : 1;
        for (int64_t lo = 0; lo <= tot; lo += step)
            for (int64_t hi = lo; hi <= tot; hi += step) check_piece(b, res, win_off, scale, unit, lo, hi);
        for (int64_t r = 0; r < n; ++r) check_piece(b, res, win_off, scale, unit, win_off[(size_t)r] * scale, win_off[(size_t)r + 1] * scale);
    }
    // the 16-bit padded layout: cleared in place (padding included: it belongs to its read) ...
    check_piece(b, res, win_off16, 1, 2, 0, win_off16[(size_t)n]);
    // ... and as the library hands it out: widened into the contiguous int32 array, then cleared
    std::vector<uint16_t> s16((size_t)win_off16[(size_t)n]);
    for (size_t i = 0; i < s16.size(); ++i) s16[i] = (uint16_t)(0xBE00u | garbage((int64_t)i));
    std::vector<int32_t> wide((size_t)nw);
    if (!wide.empty()) memset(wide.data(), 0x5A, wide.size() * 4);
    tps::widen_sums16(s16.empty() ? nullptr : s16.data(), win_off16.data(), win_off.data(), 0, n, wide.empty() ? nullptr : wide.data());
    tps::clear_skipped_windows(res.data(), win_off.data(), n, 1, 4, 0, nw, wide.empty() ? nullptr : wide.data());
    for (int64_t r = 0; r < n; ++r)
        for (int64_t w = 0; w < b.nwin[(size_t)r]; ++w) {
            const int32_t want = b.pass[(size_t)r] ? (int32_t)s16[(size_t)(win_off16[(size_t)r] + w)] : 0;
            REQUIRE(wide[(size_t)(win_off[(size_t)r] + w)] == want, "%s: widened S_w of read %lld window %lld is %d, want %d", b.name, (long long)r,
                    (long long)w, wide[(size_t)(win_off[(size_t)r] + w)], want);
        }
    // one read of the padded layout on its own (tps_batch_read_sums)
    for (int64_t r = 0; r < n; ++r) {
        std::vector<int32_t> one((size_t)b.nwin[(size_t)r]);
        tps::widen_sums16(s16.data() + win_off16[(size_t)r], win_off16.data(), win_off.data(), r, r + 1, one.empty() ? nullptr : one.data());
        tps::clear_skipped_windows(res.data(), win_off.data(), n, 1, 4, win_off[(size_t)r], win_off[(size_t)r + 1], one.empty() ? nullptr : one.data());
        for (int64_t w = 0; w < b.nwin[(size_t)r]; ++w)
            REQUIRE(one[(size_t)w] == wide[(size_t)(win_off[(size_t)r] + w)], "%s: read %lld alone differs at window %lld", b.name, (long long)r, (long long)w);
    }
}

int main() {
    const std::vector<Batch> batches = {
        {"no read passes", {3, 9, 1, 16, 8}, {0, 0, 0, 0, 0}},
        {"all reads pass", {3, 9, 1, 16, 8}, {1, 1, 1, 1, 1}},
        {"alternating", {5, 7, 8, 9, 1, 17, 2}, {1, 0, 1, 0, 1, 0, 1}},
        {"alternating, skipped first", {5, 7, 8, 9, 1, 17, 2}, {0, 1, 0, 1, 0, 1, 0}},
        {"a zero-window read between two skipped ones", {4, 6, 0, 11, 3}, {1, 0, 1, 0, 1}},
        {"zero-window reads at both ends and in a row", {0, 0, 5, 0, 0, 0, 7, 0}, {0, 1, 0, 0, 1, 0, 1, 0}},
        {"the seven-read batch", {151, 134, 151, 0, 151, 134, 151}, {1, 0, 0, 0, 1, 0, 1}},
        {"one read", {13}, {0}},
        {"no windows at all", {0, 0}, {0, 1}},
    };
    for (const Batch& b : batches) run(b);
    // no reads: nothing to clear, no pointer touched
    REQUIRE(tps::clear_skipped_windows(nullptr, nullptr, 0, 1, 4, 0, 0, nullptr) == 0, "empty batch");
    printf("ok %d batches, %d checks\n", (int)batches.size(), g_checks);
    return 0;
}
