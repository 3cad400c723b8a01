// TEST INFRASTRUCTURE ONLY -- the variant census emulation (emu_variant.cpp) as a stand-alone program for the sanitizers:
//   g++ -fsanitize=address,undefined emu_variant_main.cpp && ./a.out
// A ragged batch (reads of 50 .. 9000 bases and one 20 000-base tract, both tails, N and lower-case letters, reads without a tract,
// end beyond the read) is built in; every answer is compared with a position-by-position restatement of the rule below, so that the
// run also fails on a wrong answer, not only on a bad access.  Exit status 0 and "ok" = clean.
#include "emu_variant.cpp"

#include <algorithm>
#include <cstdio>

namespace {

int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'T' ? 2 : c == 'G' ? 3 : -1; }

// counts row and the profile's share of one read
void brute(const std::string& read, const std::string& unit, int tail, int begin, int end, int bin, int n_bins, std::vector<int64_t>& row,
           std::vector<int64_t>& prof) {
    const int m = (int)unit.size(), cols = 2 + 4 * m;
    std::string h;
    for (char c : read) h.push_back((char)(c >= 'a' && c <= 'z' ? c - 32 : c));
    if (tail) {
        std::string t(h.rbegin(), h.rend());
        for (char& c : t) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
        h = t;
    }
    end = std::min(end, (int)h.size());
    if (end - begin < m) return;
    for (int i = begin; i + m <= end; ++i) {
        const int b = std::min((end - 1 - i) / bin, n_bins - 1);
        int cls = 0;
        bool ok = true;
        for (int q = 0; q < m; ++q) ok = ok && code_of(h[(size_t)(i + q)]) >= 0;
        for (int j = 0; ok && j < m && !cls; ++j) {
            int dist = 0, at = 0;
            for (int q = 0; q < m; ++q)
                if (h[(size_t)(i + q)] != unit[(size_t)((j + q) % m)]) { if (!dist) at = q; ++dist; }
            if (dist == 0) cls = 1;
            else if (dist == 1) cls = 2 + 4 * ((j + at) % m) + code_of(h[(size_t)(i + at)]);
        }
        ++row[0]; ++prof[(size_t)b * cols];
        if (cls) { ++row[(size_t)cls]; ++prof[(size_t)b * cols + cls]; }
    }
}

uint64_t code_unit(const std::string& u) {
    uint64_t c = 0;
    for (size_t j = 0; j < u.size(); ++j) c |= (uint64_t)code_of(u[j]) << (2 * j);
    return c;
}

}  // namespace

int main() {
    const std::string units[] = {"AAAC", "CCCTAA", "CCCTAAA", "CTGTGGGGTCTGGGTG", "ACGGATGTCTAACTTCTTGGTGT", "ACGGTTCAGTCCATGACTTGCAAGTCTGATCC"};
    uint32_t x = 12345;
    auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    int checked = 0;
    for (size_t ui = 0; ui < sizeof(units) / sizeof(units[0]); ++ui) {
        const std::string& unit = units[ui];
        const int m = (int)unit.size(), cols = 2 + 4 * m;
        std::vector<std::string> reads;
        std::vector<uint8_t> tails;
        std::vector<int32_t> begin, end;
        const int lens[] = {50, 51, 63, 64, 65, 127, 129, 500, 501, 999, 1337, 2048, 4095, 4096, 4097, 8191, 9000, 20131, 3, 0};
        for (size_t li = 0; li < sizeof(lens) / sizeof(lens[0]); ++li) {
            const int L = lens[li];
            std::string r;
            const int phase = (int)(rnd() % (uint32_t)m);
            for (int i = 0; i < L; ++i) {
                char c = unit[(size_t)((phase + i) % m)];
                const uint32_t roll = rnd() % 1000u;
                if (roll < 30) c = "ACGT"[rnd() & 3];
                else if (roll < 33) c = 'N';
                else if (roll < 36) c = (char)(c + 32);
                r.push_back(c);
            }
            reads.push_back(r);
            tails.push_back((uint8_t)(rnd() & 1));
            const int b = L ? (int)(rnd() % (uint32_t)std::min(L, 120)) : 0;
            int e = li % 3 == 0 ? L : li % 3 == 1 ? L + 9 : b + (int)(rnd() % (uint32_t)(L - b + 1));
            if (li % 7 == 3) { begin.push_back(0); end.push_back(0); continue; }
            begin.push_back(b);
            end.push_back(std::max(e, b));
        }
        std::vector<uint8_t> bases;
        std::vector<int64_t> offsets{0};
        for (const std::string& r : reads) {
            bases.insert(bases.end(), r.begin(), r.end());
            offsets.push_back((int64_t)bases.size());
        }
        bases.push_back(0);
        const int64_t n = (int64_t)reads.size();
        const int prm[][2] = {{500, 40}, {64, 3}, {4064, 2}, {64, 64}, {100, 1}};
        for (size_t p = 0; p < sizeof(prm) / sizeof(prm[0]); ++p) {
            const int bin = prm[p][0], n_bins = prm[p][1];
            std::vector<uint32_t> counts((size_t)(n * cols));
            std::vector<int64_t> profile((size_t)(n_bins * cols));
            const bool with_prof = p != 1 || ui != 0;                          // (profile = NULL once)
            const int rc = emu_variant_census(bases.data(), offsets.data(), n, code_unit(unit), m, tails.data(), begin.data(), end.data(), n, bin, n_bins,
                                              (int)((p + ui) & 3), counts.data(), n * cols, with_prof ? profile.data() : nullptr, with_prof ? n_bins * cols : 0);
            if (rc != TPS_OK) { printf("unit %zu, parameter set %zu: rc %d (%s)\n", ui, p, rc, emu_variant_last_error()); return 1; }
            std::vector<int64_t> wprof((size_t)(n_bins * cols), 0);
            for (int64_t r = 0; r < n; ++r) {
                std::vector<int64_t> row((size_t)cols, 0);
                brute(reads[(size_t)r], unit, tails[(size_t)r], begin[(size_t)r], end[(size_t)r], bin, n_bins, row, wprof);
                for (int c = 0; c < cols; ++c)
                    if ((int64_t)counts[(size_t)(r * cols + c)] != row[(size_t)c]) {
                        printf("unit %zu, parameter set %zu, read %lld, column %d: got %u, want %lld\n", ui, p, (long long)r, c, counts[(size_t)(r * cols + c)],
                               (long long)row[(size_t)c]);
                        return 1;
                    }
                ++checked;
            }
            if (with_prof && profile != wprof) { printf("unit %zu, parameter set %zu: the profile differs\n", ui, p); return 1; }
        }
    }
    // the refusals, and an empty batch
    const uint8_t t0[1] = {0}, t2[1] = {2};
    const int32_t b0[1] = {0}, e0[1] = {3}, neg[1] = {-1};
    const uint8_t one_read[4] = {'A', 'C', 'G', 'T'};
    const int64_t off[2] = {0, 3};
    uint32_t cnt[2 + 4 * 32];
    const uint64_t u6 = code_unit("CCCTAA");
    if (emu_variant_census(one_read, off, 1, u6, 1, t0, b0, e0, 1, 500, 40, 0, cnt, 6, nullptr, 0) != TPS_E_ARG) return 1;
    if (emu_variant_census(one_read, off, 1, u6, 33, t0, b0, e0, 1, 500, 40, 0, cnt, 134, nullptr, 0) != TPS_E_ARG) return 1;
    if (emu_variant_census(one_read, off, 1, code_unit("CCACCA"), 6, t0, b0, e0, 1, 500, 40, 0, cnt, 26, nullptr, 0) != TPS_E_ARG) return 1;
    if (emu_variant_census(one_read, off, 1, u6, 6, t2, b0, e0, 1, 500, 40, 0, cnt, 26, nullptr, 0) != TPS_E_ARG) return 1;
    if (emu_variant_census(one_read, off, 1, u6, 6, t0, neg, e0, 1, 500, 40, 0, cnt, 26, nullptr, 0) != TPS_E_ARG) return 1;
    if (emu_variant_census(one_read, off, 1, u6, 6, t0, e0, b0, 1, 500, 40, 0, cnt, 26, nullptr, 0) != TPS_E_ARG) return 1;
    if (emu_variant_census(one_read, off, 1, u6, 6, t0, b0, e0, 1, 63, 40, 0, cnt, 26, nullptr, 0) != TPS_E_CAPACITY) return 1;
    if (emu_variant_census(one_read, off, 1, u6, 6, t0, b0, e0, 1, 4065, 40, 0, cnt, 26, nullptr, 0) != TPS_E_CAPACITY) return 1;
    if (emu_variant_census(one_read, off, 1, u6, 6, t0, b0, e0, 1, 500, 65, 0, cnt, 26, nullptr, 0) != TPS_E_CAPACITY) return 1;
    if (emu_variant_census(one_read, off, 0, u6, 6, nullptr, nullptr, nullptr, 0, 500, 40, 0, nullptr, 0, nullptr, 0) != TPS_OK) return 1;
    printf("ok %d reads\n", checked);
    return 0;
}
