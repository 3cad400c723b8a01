// TEST INFRASTRUCTURE ONLY -- the boundary refinement emulation (emu_refine.cpp) as a stand-alone program for the sanitizers:
//   g++ -fsanitize=address,undefined emu_refine_main.cpp && ./a.out CASES
// CASES is a text file (tests/test_refine.py writes the cases of tests/refine_cases.py into it), one case after another:
//   rcase <unit> <hit> <miss> <sep> <n_reads>
//   <tail> <begin> <end> <at> <read>     n_reads lines; "-" is the empty read
// Every row is compared with the plain rule below (strings, a vector of prefix sums), so that the run also fails on a wrong answer,
// not only on a bad access.  The staging area is one wave's, poisoned, and the table and the rows have exactly their sizes
// (emu_boundary_refine).  Without an argument a small built-in batch runs.  Exit status 0 and "ok" = clean.
#include "emu_refine.cpp"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <set>
#include <sstream>

namespace {

int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'T' ? 2 : c == 'G' ? 3 : -1; }

std::string revcomp(const std::string& u) {
    std::string t(u.rbegin(), u.rend());
    for (char& c : t) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
    return t;
}

struct Read { std::string seq; int tail, begin, end, at; };

std::set<std::string> word_set(const std::string& unit) {
    const size_t m = unit.size(), w = std::min<size_t>(m, 8);
    std::string rep;
    while (rep.size() < m + w) rep += unit;
    std::set<std::string> out;
    for (size_t j = 0; j < m; ++j) {
        const std::string word = rep.substr(j, w);
        for (size_t q = 0; q < w; ++q)
            for (char c : std::string("ACGT")) {
                std::string v = word;
                v[q] = c;
                out.insert(v);
            }
    }
    return out;
}

tps_refine brute(const Read& rd, const std::set<std::string>& words, int w, int hit, int miss, int sep) {
    std::string h;
    for (char c : rd.seq) h.push_back((char)(c >= 'a' && c <= 'z' ? c - 32 : c));
    if (rd.tail) h = revcomp(h);
    const long e = std::min((long)rd.end, (long)h.size());
    const long n = e - rd.begin - w + 1;
    tps_refine out{rd.begin, 0, 0, 0, 0, 0, 0, -1};
    if (n <= 0) return out;
    std::vector<int> x((size_t)n), P((size_t)n + 1, 0);
    for (long i = 0; i < n; ++i) {
        x[(size_t)i] = words.count(h.substr((size_t)(rd.begin + i), (size_t)w)) ? 1 : 0;
        P[(size_t)i + 1] = P[(size_t)i] + (x[(size_t)i] ? hit : -miss);
    }
    long rel = 0;
    for (long j = 1; j <= n; ++j) if (P[(size_t)j] > P[(size_t)rel]) rel = j;
    long run = -1;
    for (long j = 0; j <= n; ++j)
        if (std::labs(j - rel) >= sep && (run < 0 || P[(size_t)j] > P[(size_t)run])) run = j;
    const long at = std::min(std::max((long)rd.at, (long)rd.begin), rd.begin + n) - rd.begin;
    int before = 0, all = 0;
    for (long i = 0; i < n; ++i) { all += x[(size_t)i]; if (i < rel) before += x[(size_t)i]; }
    out.pos = (int32_t)(rd.begin + rel);
    out.score = P[(size_t)rel];
    out.drop = P[(size_t)rel] - P[(size_t)n];
    out.at_score = P[(size_t)at];
    out.hits_before = before;
    out.hits_after = all - before;
    if (run >= 0) { out.runner = P[(size_t)run]; out.runner_pos = (int32_t)(rd.begin + run); }
    return out;
}

uint64_t unit_code(const std::string& unit) {
    uint64_t c = 0;
    for (size_t i = 0; i < unit.size() && i < 32; ++i) c |= (uint64_t)code_of(unit[i]) << (2 * i);
    return c;
}

int run_case(const std::string& unit, int hit, int miss, int sep, const std::vector<Read>& reads, int shift, long& checked) {
    std::vector<uint8_t> bases, tails;
    std::vector<int64_t> offsets{0};
    std::vector<int32_t> begin, end, at;
    for (const Read& r : reads) {
        bases.insert(bases.end(), r.seq.begin(), r.seq.end());
        offsets.push_back((int64_t)bases.size());
        tails.push_back((uint8_t)r.tail); begin.push_back(r.begin); end.push_back(r.end); at.push_back(r.at);
    }
    bases.push_back(0);
    const int64_t n = (int64_t)reads.size();
    std::vector<tps_refine> rows((size_t)n);                    // exactly the rows
    const int rc = emu_boundary_refine(bases.data(), offsets.data(), n, unit_code(unit), (int)unit.size(), tails.data(), begin.data(), end.data(), at.data(), n,
                                       hit, miss, sep, shift, rows.data(), n);
    if (rc != TPS_OK) { printf("rc %d (%s)\n", rc, emu_refine_last_error()); return 1; }
    const std::set<std::string> words = word_set(unit);
    const int w = (int)std::min<size_t>(unit.size(), 8);
    for (int64_t r = 0; r < n; ++r) {
        const tps_refine want = brute(reads[(size_t)r], words, w, hit, miss, sep);
        if (memcmp(&want, &rows[(size_t)r], sizeof want) != 0) {
            const tps_refine& g = rows[(size_t)r];
            printf("read %lld: got (%d %d %d %d %d %d %d %d), want (%d %d %d %d %d %d %d %d)\n", (long long)r, g.pos, g.score, g.drop, g.at_score, g.hits_before,
                   g.hits_after, g.runner, g.runner_pos, want.pos, want.score, want.drop, want.at_score, want.hits_before, want.hits_after, want.runner, want.runner_pos);
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
            int hit, miss, sep;
            long n;
            if (!(hd >> tag >> unit >> hit >> miss >> sep >> n) || tag != "rcase") { printf("bad case line: %s\n", line.c_str()); return 1; }
            std::vector<Read> reads;
            for (long i = 0; i < n; ++i) {
                if (!std::getline(in, line)) { printf("the file ends inside a case\n"); return 1; }
                std::istringstream rl(line);
                Read r;
                if (!(rl >> r.tail >> r.begin >> r.end >> r.at >> r.seq)) { printf("bad read line\n"); return 1; }
                if (r.seq == "-") r.seq.clear();
                reads.push_back(r);
            }
            if (run_case(unit, hit, miss, sep, reads, n_cases & 3, checked)) return 1;
            ++n_cases;
        }
    } else {
        uint32_t x = 4321;
        auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
        const char* units[] = {"CCCTAA", "AAAC", "ACGGATGTCTAACTTCTTGGTGT", "ACGGTTCAGTCCATGACTTGCAAGTCTGATCC"};
        for (const char* u : units) {
            const std::string unit(u);
            std::vector<Read> reads;
            const int lens[] = {0, 1, 7, 8, 63, 64, 71, 72, 73, 500, 4031, 4039, 4040, 4041, 9000, 20000};
            for (int L : lens) {
                // a tract of noisy repeats, then random letters; now and then an N or a lower-case letter
                const int tract = L / 3;
                std::string h;
                for (int i = 0; i < L; ++i) {
                    char c = i < tract && rnd() % 10u != 0 ? unit[(size_t)i % unit.size()] : "ACGT"[rnd() & 3];
                    if (rnd() % 400u == 0) c = 'N';
                    h.push_back(c);
                }
                const int tail = (int)(rnd() & 1);
                std::string s = tail ? revcomp(h) : h;
                if (L == 500) for (char& c : s) c = (char)(c + 32);            // lower case
                const int b = (int)(rnd() % 40u);
                reads.push_back(Read{s, tail, b, b + (int)(rnd() % (unsigned)(L + 100)), (int)(rnd() % (unsigned)(L + 50))});
            }
            if (run_case(unit, 2, 1, 200, reads, n_cases & 3, checked)) return 1;
            ++n_cases;
            if (run_case(unit, 1, 16, 1, reads, n_cases & 3, checked)) return 1;
            ++n_cases;
        }
    }
    // the refusals, and an empty batch
    const uint8_t one_read[12] = {'C', 'C', 'C', 'T', 'A', 'A', 'C', 'C', 'C', 'T', 'A', 'A'};
    const int64_t off[2] = {0, 12};
    const uint64_t U = unit_code("CCCTAA");
    tps_refine row[1];
    auto call = [&](uint64_t unit, int m, int tail, int b, int e, int at, int hit, int miss, int sep, int64_t nr, int64_t ol) {
        const uint8_t t[1] = {(uint8_t)tail};
        const int32_t bb[1] = {b}, ee[1] = {e}, aa[1] = {at};
        return emu_boundary_refine(one_read, off, 1, unit, m, t, bb, ee, aa, nr, hit, miss, sep, 0, row, ol);
    };
    if (call(U, 6, 0, 0, 12, 3, 2, 1, 200, 1, 1) != TPS_OK || row[0].pos != 7 || row[0].score != 14 || row[0].drop != 0 || row[0].at_score != 6 || row[0].runner_pos != -1) return 1;
    if (call(U, 3, 0, 0, 12, 3, 2, 1, 200, 1, 1) != TPS_E_ARG || call(unit_code("CCACCA"), 6, 0, 0, 12, 3, 2, 1, 200, 1, 1) != TPS_E_ARG) return 1;
    if (call(U, 6, 2, 0, 12, 3, 2, 1, 200, 1, 1) != TPS_E_ARG || call(U, 6, 0, -1, 12, 3, 2, 1, 200, 1, 1) != TPS_E_ARG || call(U, 6, 0, 5, 4, 3, 2, 1, 200, 1, 1) != TPS_E_ARG) return 1;
    if (call(U, 6, 0, 0, 12, -1, 2, 1, 200, 1, 1) != TPS_E_ARG || call(U, 6, 0, 0, 12, 3, 2, 1, 200, 2, 1) != TPS_E_ARG || call(U, 6, 0, 0, 12, 3, 2, 1, 200, 1, 2) != TPS_E_ARG) return 1;
    if (call(U, 6, 0, 0, 12, 3, 0, 1, 200, 1, 1) != TPS_E_CAPACITY || call(U, 6, 0, 0, 12, 3, 17, 1, 200, 1, 1) != TPS_E_CAPACITY) return 1;
    if (call(U, 6, 0, 0, 12, 3, 2, 0, 200, 1, 1) != TPS_E_CAPACITY || call(U, 6, 0, 0, 12, 3, 2, 17, 200, 1, 1) != TPS_E_CAPACITY) return 1;
    if (call(U, 6, 0, 0, 12, 3, 2, 1, 0, 1, 1) != TPS_E_CAPACITY || call(U, 6, 0, 0, 12, 3, 2, 1, 65536, 1, 1) != TPS_E_CAPACITY) return 1;
    if (call(U, 6, 0, 0, 1 << 30, 3, 16, 16, 65535, 1, 1) != TPS_OK) return 1;                   // (end far past the read: clamped before it is measured)
    if (emu_boundary_refine(one_read, off, 0, U, 6, nullptr, nullptr, nullptr, nullptr, 0, 2, 1, 200, 0, nullptr, 0) != TPS_OK) return 1;
    printf("ok %d cases, %ld rows\n", n_cases, checked);
    return 0;
}
