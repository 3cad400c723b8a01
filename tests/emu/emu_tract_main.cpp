// TEST INFRASTRUCTURE ONLY -- the tract map emulation (emu_tract.cpp) as a stand-alone program for the sanitizers:
//   g++ -fsanitize=address,undefined emu_tract_main.cpp && ./a.out CASES
// CASES is a text file (tests/test_tract_map.py writes the cases of tests/tract_cases.py into it), one case after another:
//   case <unit> <block> <min_hits> <gap> <min_blocks> <max_tracts> <n_reads>
//   <read>                                  n_reads lines; "-" is the empty read
// Every answer is compared with a position-by-position restatement of the rule below, so that the run also fails on a wrong answer,
// not only on a bad access.  Without an argument a small built-in batch runs.  Exit status 0 and "ok" = clean.
#include "emu_tract.cpp"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

namespace {

int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'T' ? 2 : c == 'G' ? 3 : -1; }

uint64_t code_unit(const std::string& u) {
    uint64_t c = 0;
    for (size_t j = 0; j < u.size(); ++j) c |= (uint64_t)code_of(u[j]) << (2 * j);
    return c;
}

std::string revcomp(const std::string& u) {
    std::string t(u.rbegin(), u.rend());
    for (char& c : t) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return t;
}

// is h[i .. i + w) within one substitution of a cyclic word of u?
bool hit(const std::string& h, size_t i, const std::string& u, int w) {
    const int m = (int)u.size();
    for (int q = 0; q < w; ++q)
        if (code_of(h[i + (size_t)q]) < 0) return false;
    for (int j = 0; j < m; ++j) {
        int dist = 0;
        for (int q = 0; q < w; ++q) dist += h[i + (size_t)q] != u[(size_t)((j + q) % m)];
        if (dist <= 1) return true;
    }
    return false;
}

struct Want {
    std::vector<tps_tract> tracts;      // the first max_tracts, zero-filled
    int found;
    uint32_t hits, flagged;
};

Want brute(const std::string& read, const std::string& u, int block, int min_hits, int gap, int min_blocks, int max_tracts) {
    const int w = std::min((int)u.size(), 8);
    std::string h;
    for (char c : read) h.push_back((char)(c >= 'a' && c <= 'z' ? c - 32 : c));
    const long L = (long)h.size(), npos = L - w + 1;
    Want out{std::vector<tps_tract>((size_t)max_tracts, tps_tract{0, 0, 0, 0}), 0, 0, 0};
    std::vector<int> count;
    for (long i = 0; i < npos; ++i) {
        if (i % block == 0) count.push_back(0);
        if (hit(h, (size_t)i, u, w)) { ++count.back(); ++out.hits; }
    }
    const long nb = (long)count.size();
    long j = 0;
    while (j < nb) {
        if (count[(size_t)j] < min_hits) { ++j; continue; }
        long b = j, last = j;
        for (long k = j + 1; k < nb && k - last <= gap + 1; ++k)
            if (count[(size_t)k] >= min_hits) last = k;
        const long e = last + 1;
        if (e - b >= min_blocks) {
            if (out.found < max_tracts) {
                int hits = 0;
                for (long k = b; k < e; ++k) hits += count[(size_t)k];
                out.tracts[(size_t)out.found] = tps_tract{(int32_t)(b * block), (int32_t)std::min(e * block + w - 1, L), hits, (int32_t)(e - b)};
            }
            ++out.found;
        }
        j = e;
    }
    for (int c : count) out.flagged += c >= min_hits;
    return out;
}

int run_case(const std::string& unit, int block, int min_hits, int gap, int min_blocks, int max_tracts, const std::vector<std::string>& reads, int shift,
             long& checked) {
    std::vector<uint8_t> bases;
    std::vector<int64_t> offsets{0};
    for (const std::string& r : reads) {
        bases.insert(bases.end(), r.begin(), r.end());
        offsets.push_back((int64_t)bases.size());
    }
    bases.push_back(0);
    const int64_t n = (int64_t)reads.size();
    std::vector<tps_tract> tracts((size_t)(n * 2 * max_tracts));
    std::vector<int32_t> found((size_t)(n * 2));
    std::vector<uint32_t> totals((size_t)(n * 4));
    const int rc = emu_tract_map(bases.data(), offsets.data(), n, code_unit(unit), (int)unit.size(), block, min_hits, gap, min_blocks, max_tracts, shift,
                                 tracts.data(), n * 2 * max_tracts, found.data(), n * 2, totals.data(), n * 4);
    if (rc != TPS_OK) { printf("unit %s: rc %d (%s)\n", unit.c_str(), rc, emu_tract_last_error()); return 1; }
    for (int64_t r = 0; r < n; ++r)
        for (int s = 0; s < 2; ++s) {
            const Want w = brute(reads[(size_t)r], s ? revcomp(unit) : unit, block, min_hits, gap, min_blocks, max_tracts);
            bool same = found[(size_t)(r * 2 + s)] == w.found && totals[(size_t)(r * 4 + s)] == w.hits && totals[(size_t)(r * 4 + 2 + s)] == w.flagged;
            for (int t = 0; t < max_tracts; ++t) {
                const tps_tract &g = tracts[(size_t)((r * 2 + s) * max_tracts + t)], &x = w.tracts[(size_t)t];
                same = same && g.begin == x.begin && g.end == x.end && g.hits == x.hits && g.blocks == x.blocks;
            }
            if (!same) {
                printf("unit %s block %d min_hits %d gap %d min_blocks %d max_tracts %d, read %lld strand %d: got found %d hits %u, want found %d hits %u\n", unit.c_str(),
                       block, min_hits, gap, min_blocks, max_tracts, (long long)r, s, found[(size_t)(r * 2 + s)], totals[(size_t)(r * 4 + s)], w.found, w.hits);
                return 1;
            }
            ++checked;
        }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    long checked = 0;
    int n_cases = 0;
    if (argc > 1) {
        std::ifstream in(argv[1]);
        if (!in) { printf("cannot read %s\n", argv[1]); return 1; }
        std::string line;
        while (std::getline(in, line)) {
            if (line.empty()) continue;
            std::istringstream hd(line);
            std::string tag, unit;
            int block, min_hits, gap, min_blocks, max_tracts;
            long n;
            if (!(hd >> tag >> unit >> block >> min_hits >> gap >> min_blocks >> max_tracts >> n) || tag != "case") { printf("bad case line: %s\n", line.c_str()); return 1; }
            std::vector<std::string> reads;
            for (long i = 0; i < n; ++i) {
                if (!std::getline(in, line)) { printf("the file ends inside a case\n"); return 1; }
                reads.push_back(line == "-" ? std::string() : line);
            }
            if (run_case(unit, block, min_hits, gap, min_blocks, max_tracts, reads, n_cases & 3, checked)) return 1;
            ++n_cases;
        }
    } else {
        uint32_t x = 12345;
        auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
        const std::string units[] = {"AAAC", "CCCTAA", "CTGTGGGGTCTGGGTG", "ACGGTTCAGTCCATGACTTGCAAGTCTGATCC"};
        for (const std::string& unit : units) {
            std::vector<std::string> reads;
            const int lens[] = {0, 3, 7, 8, 9, 71, 72, 500, 4039, 4040, 4041, 9000};
            for (int L : lens) {
                std::string r;
                for (int i = 0; i < L; ++i) {
                    const bool tel = (i / 700) % 2 == 0;
                    char c = tel ? unit[(size_t)i % unit.size()] : "ACGT"[rnd() & 3];
                    if (rnd() % 500u == 0) c = 'N';
                    r.push_back(c);
                }
                reads.push_back(r);
            }
            if (run_case(unit, 64, 20, 1, 2, 8, reads, n_cases & 3, checked)) return 1;
            if (run_case(unit, 1024, 300, 0, 1, 1, reads, n_cases & 3, checked)) return 1;
            ++n_cases;
        }
    }
    // the refusals, and an empty batch
    const uint8_t one_read[4] = {'A', 'C', 'G', 'T'};
    const int64_t off[2] = {0, 3};
    tps_tract tr[2 * 16];
    int32_t fo[2];
    uint32_t to[4];
    const uint64_t u6 = code_unit("CCCTAA");
    auto call = [&](uint64_t unit, int m, int block, int min_hits, int gap, int min_blocks, int max_tracts, int64_t tl) {
        return emu_tract_map(one_read, off, 1, unit, m, block, min_hits, gap, min_blocks, max_tracts, 0, tr, tl, fo, 2, to, 4);
    };
    if (call(u6, 6, 64, 20, 1, 2, 8, 16) != TPS_OK) return 1;
    if (call(u6, 3, 64, 20, 1, 2, 8, 16) != TPS_E_ARG || call(u6, 33, 64, 20, 1, 2, 8, 16) != TPS_E_ARG) return 1;
    if (call(code_unit("CCACCA"), 6, 64, 20, 1, 2, 8, 16) != TPS_E_ARG || call(u6 | (1ull << 12), 6, 64, 20, 1, 2, 8, 16) != TPS_E_ARG) return 1;
    if (call(u6, 6, 64, 20, 1, 2, 8, 15) != TPS_E_ARG) return 1;
    if (call(u6, 6, 96, 20, 1, 2, 8, 16) != TPS_E_CAPACITY || call(u6, 6, 0, 20, 1, 2, 8, 16) != TPS_E_CAPACITY || call(u6, 6, 1088, 20, 1, 2, 8, 16) != TPS_E_CAPACITY) return 1;
    if (call(u6, 6, 64, 0, 1, 2, 8, 16) != TPS_E_CAPACITY || call(u6, 6, 64, 65, 1, 2, 8, 16) != TPS_E_CAPACITY) return 1;
    if (call(u6, 6, 64, 20, -1, 2, 8, 16) != TPS_E_CAPACITY || call(u6, 6, 64, 20, 65, 2, 8, 16) != TPS_E_CAPACITY) return 1;
    if (call(u6, 6, 64, 20, 1, 0, 8, 16) != TPS_E_CAPACITY || call(u6, 6, 64, 20, 1, 65, 8, 16) != TPS_E_CAPACITY) return 1;
    if (call(u6, 6, 64, 20, 1, 2, 0, 0) != TPS_E_CAPACITY || call(u6, 6, 64, 20, 1, 2, 17, 34) != TPS_E_CAPACITY) return 1;
    if (emu_tract_map(one_read, off, 0, u6, 6, 64, 20, 1, 2, 8, 0, nullptr, 0, nullptr, 0, nullptr, 0) != TPS_OK) return 1;
    printf("ok %d cases, %ld read strands\n", n_cases, checked);
    return 0;
}
