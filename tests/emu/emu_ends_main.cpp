// TEST INFRASTRUCTURE ONLY -- the end sketch and link emulation (emu_ends.cpp) as a stand-alone program for the sanitizers:
//   g++ -fsanitize=address,undefined emu_ends_main.cpp && ./a.out CASES
// CASES is a text file (tests/test_end_sketch.py writes the cases of tests/ends_cases.py into it), one case after another:
//   case <unit> <k> <buckets> <n_reads>
//   <tail> <begin> <end> <read>             n_reads lines; "-" is the empty read
// Every sketch is compared with a position-by-position restatement of the rule below, and the sketches of every case are linked
// (min_match 1 and 3, max_links 2 and 256) and compared with an all-pairs loop, so that the run also fails on a wrong answer, not
// only on a bad access.  Without an argument a small built-in batch runs.  Exit status 0 and "ok" = clean.
#include "emu_ends.cpp"

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
    for (char& c : t) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
    return t;
}

// is h[i .. i + w) within one substitution of a cyclic word of u?
bool near(const std::string& h, size_t i, const std::string& u, int w) {
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

uint32_t fmix(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

struct Read { std::string seq; int tail, begin, end; };

void brute_sketch(const Read& rd, const std::string& unit, int k, int B, std::vector<uint32_t>& row, uint32_t& kept) {
    const int w = std::min((int)unit.size(), 8);
    std::string h;
    for (char c : rd.seq) h.push_back((char)(c >= 'a' && c <= 'z' ? c - 32 : c));
    if (rd.tail) h = revcomp(h);
    const std::string rc = revcomp(unit);
    const long e = std::min((long)rd.end, (long)h.size());
    int lg = 0;
    while ((1 << lg) < B) ++lg;
    row.assign((size_t)B, 0xFFFFFFFFu);
    kept = 0;
    for (long i = rd.begin; i + k <= e; ++i) {
        bool ok = true;
        uint32_t c = 0;
        for (int q = 0; q < k && ok; ++q) {
            const int v = code_of(h[(size_t)(i + q)]);
            if (v < 0) ok = false; else c |= (uint32_t)v << (2 * q);
        }
        for (int d = 0; d <= k - w && ok; ++d)
            if (near(h, (size_t)(i + d), unit, w) || near(h, (size_t)(i + d), rc, w)) ok = false;
        if (!ok) continue;
        ++kept;
        const uint32_t x = fmix(c ^ 0x9E3779B9u);
        row[x >> (32 - lg)] = std::min(row[x >> (32 - lg)], x);
    }
}

int check_links(const std::vector<uint32_t>& sk, int64_t n, int B, int min_match, int max_links, long& checked) {
    std::vector<int32_t> degree((size_t)n), links((size_t)(n * max_links)), matches((size_t)(n * max_links));
    const int rc = emu_sketch_links(sk.data(), n, B, n * B, min_match, max_links, degree.data(), n, links.data(), n * max_links, matches.data(), n * max_links);
    if (rc != TPS_OK) { printf("links: rc %d (%s)\n", rc, emu_ends_last_error()); return 1; }
    for (int64_t i = 0; i < n; ++i) {
        int found = 0;
        for (int64_t j = i + 1; j < n; ++j) {
            int mt = 0;
            for (int b = 0; b < B; ++b) mt += sk[(size_t)(i * B + b)] == sk[(size_t)(j * B + b)] && sk[(size_t)(i * B + b)] != 0xFFFFFFFFu;
            if (mt < min_match) continue;
            if (found < max_links && (links[(size_t)(i * max_links + found)] != j || matches[(size_t)(i * max_links + found)] != mt)) {
                printf("links of row %lld, place %d: got %d (%d), want %lld (%d)\n", (long long)i, found, links[(size_t)(i * max_links + found)],
                       matches[(size_t)(i * max_links + found)], (long long)j, mt);
                return 1;
            }
            ++found;
        }
        if (degree[(size_t)i] != found) { printf("degree of row %lld: got %d, want %d\n", (long long)i, degree[(size_t)i], found); return 1; }
        for (int p = found; p < max_links; ++p)
            if (links[(size_t)(i * max_links + p)] != -1 || matches[(size_t)(i * max_links + p)] != 0) { printf("row %lld is not -1 / 0 behind its links\n", (long long)i); return 1; }
        ++checked;
    }
    return 0;
}

int run_case(const std::string& unit, int k, int B, const std::vector<Read>& reads, int shift, long& checked) {
    std::vector<uint8_t> bases, tails;
    std::vector<int64_t> offsets{0};
    std::vector<int32_t> begin, end;
    for (const Read& r : reads) {
        bases.insert(bases.end(), r.seq.begin(), r.seq.end());
        offsets.push_back((int64_t)bases.size());
        tails.push_back((uint8_t)r.tail); begin.push_back(r.begin); end.push_back(r.end);
    }
    bases.push_back(0);
    const int64_t n = (int64_t)reads.size();
    std::vector<uint32_t> sk((size_t)(n * B)), kept((size_t)n);
    const int rc = emu_end_sketch(bases.data(), offsets.data(), n, code_unit(unit), (int)unit.size(), k, B, tails.data(), begin.data(), end.data(), n, shift,
                                  sk.data(), n * B, kept.data(), n);
    if (rc != TPS_OK) { printf("unit %s: rc %d (%s)\n", unit.c_str(), rc, emu_ends_last_error()); return 1; }
    for (int64_t r = 0; r < n; ++r) {
        std::vector<uint32_t> row;
        uint32_t kp;
        brute_sketch(reads[(size_t)r], unit, k, B, row, kp);
        if (kp != kept[(size_t)r] || !std::equal(row.begin(), row.end(), sk.begin() + r * B)) {
            printf("unit %s k %d buckets %d, read %lld: got kept %u, want %u\n", unit.c_str(), k, B, (long long)r, kept[(size_t)r], kp);
            return 1;
        }
        ++checked;
    }
    if (check_links(sk, n, B, 1, 2, checked) || check_links(sk, n, B, 3, 256, checked)) return 1;
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
            int k, B;
            long n;
            if (!(hd >> tag >> unit >> k >> B >> n) || tag != "case") { printf("bad case line: %s\n", line.c_str()); return 1; }
            std::vector<Read> reads;
            for (long i = 0; i < n; ++i) {
                if (!std::getline(in, line)) { printf("the file ends inside a case\n"); return 1; }
                std::istringstream rl(line);
                Read r;
                if (!(rl >> r.tail >> r.begin >> r.end >> r.seq)) { printf("bad read line\n"); return 1; }
                if (r.seq == "-") r.seq.clear();
                reads.push_back(r);
            }
            if (run_case(unit, k, B, reads, n_cases & 3, checked)) return 1;
            ++n_cases;
        }
    } else {
        uint32_t x = 12345;
        auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
        const std::string units[] = {"AAAC", "CCCTAA", "CTGTGGGGTCTGGGTG", "ACGGTTCAGTCCATGACTTGCAAGTCTGATCC"};
        for (const std::string& unit : units) {
            std::vector<Read> reads;
            std::string sub;                       // one subtelomere shared by the reads: their sketches link
            for (int i = 0; i < 9000; ++i) sub.push_back("ACGT"[rnd() & 3]);
            const int lens[] = {0, 3, 11, 12, 13, 75, 76, 500, 3979, 3980, 3981, 9000};
            for (int L : lens) {
                std::string r;
                for (int i = 0; i < L; ++i) {
                    char c = i < 300 ? unit[(size_t)i % unit.size()] : sub[(size_t)i];
                    if (rnd() % 500u == 0) c = 'N';
                    if (rnd() % 40u == 0) c = "ACGT"[rnd() & 3];
                    r.push_back(c);
                }
                const int tail = (int)(rnd() & 1);
                reads.push_back(Read{tail ? revcomp(r) : r, tail, L > 400 ? 250 : 0, L > 400 ? L + 7 : L});
            }
            if (run_case(unit, 12, 256, reads, n_cases & 3, checked)) return 1;
            if (run_case(unit, 8, 64, reads, n_cases & 3, checked) || run_case(unit, 16, 512, reads, n_cases & 3, checked)) return 1;
            ++n_cases;
        }
    }
    // the refusals, and an empty batch
    const uint8_t one_read[4] = {'A', 'C', 'G', 'T'};
    const int64_t off[2] = {0, 3};
    uint32_t sk[512], kp[1];
    const uint64_t u6 = code_unit("CCCTAA");
    auto call = [&](uint64_t unit, int m, int k, int B, int tail, int b, int e, int64_t nr, int64_t sl, int64_t kl) {
        const uint8_t t[1] = {(uint8_t)tail};
        const int32_t bb[1] = {b}, ee[1] = {e};
        return emu_end_sketch(one_read, off, 1, unit, m, k, B, t, bb, ee, nr, 0, sk, sl, kp, kl);
    };
    if (call(u6, 6, 12, 256, 0, 0, 3, 1, 256, 1) != TPS_OK || kp[0] != 0 || sk[0] != 0xFFFFFFFFu || sk[255] != 0xFFFFFFFFu) return 1;
    if (call(u6, 3, 12, 256, 0, 0, 3, 1, 256, 1) != TPS_E_ARG || call(u6, 33, 12, 256, 0, 0, 3, 1, 256, 1) != TPS_E_ARG) return 1;
    if (call(code_unit("CCACCA"), 6, 12, 256, 0, 0, 3, 1, 256, 1) != TPS_E_ARG || call(u6 | (1ull << 12), 6, 12, 256, 0, 0, 3, 1, 256, 1) != TPS_E_ARG) return 1;
    if (call(u6, 6, 7, 256, 0, 0, 3, 1, 256, 1) != TPS_E_CAPACITY || call(u6, 6, 17, 256, 0, 0, 3, 1, 256, 1) != TPS_E_CAPACITY) return 1;
    if (call(u6, 6, 12, 32, 0, 0, 3, 1, 32, 1) != TPS_E_ARG || call(u6, 6, 12, 192, 0, 0, 3, 1, 192, 1) != TPS_E_ARG || call(u6, 6, 12, 1024, 0, 0, 3, 1, 1024, 1) != TPS_E_ARG) return 1;
    if (call(u6, 6, 12, 256, 2, 0, 3, 1, 256, 1) != TPS_E_ARG || call(u6, 6, 12, 256, 0, -1, 3, 1, 256, 1) != TPS_E_ARG || call(u6, 6, 12, 256, 0, 4, 3, 1, 256, 1) != TPS_E_ARG) return 1;
    if (call(u6, 6, 12, 256, 0, 0, 16385, 1, 256, 1) != TPS_E_CAPACITY || call(u6, 6, 12, 256, 0, 0, 16384, 1, 256, 1) != TPS_OK) return 1;
    if (call(u6, 6, 12, 256, 0, 0, 3, 2, 256, 1) != TPS_E_ARG || call(u6, 6, 12, 256, 0, 0, 3, 1, 255, 1) != TPS_E_ARG || call(u6, 6, 12, 256, 0, 0, 3, 1, 256, 2) != TPS_E_ARG) return 1;
    if (emu_end_sketch(one_read, off, 0, u6, 6, 12, 256, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, 0) != TPS_OK) return 1;
    int32_t dg[2], ln[2 * 256], mt[2 * 256];
    uint32_t two[2 * 64];
    for (int i = 0; i < 128; ++i) two[i] = (uint32_t)(i % 64);
    auto lcall = [&](int64_t n, int B, int64_t sl, int mm, int ml, int64_t dl, int64_t ll, int64_t tl) { return emu_sketch_links(two, n, B, sl, mm, ml, dg, dl, ln, ll, mt, tl); };
    if (lcall(2, 64, 128, 64, 256, 2, 512, 512) != TPS_OK || dg[0] != 1 || dg[1] != 0 || ln[0] != 1 || mt[0] != 64 || ln[1] != -1) return 1;
    if (lcall(2, 32, 64, 6, 4, 2, 8, 8) != TPS_E_ARG || lcall(2, 64, 127, 6, 4, 2, 8, 8) != TPS_E_ARG || lcall(2, 64, 128, 6, 4, 1, 8, 8) != TPS_E_ARG) return 1;
    if (lcall(2, 64, 128, 6, 4, 2, 7, 8) != TPS_E_ARG || lcall(2, 64, 128, 6, 4, 2, 8, 9) != TPS_E_ARG) return 1;
    if (lcall(262145, 64, 262145ll * 64, 6, 4, 262145, 262145ll * 4, 262145ll * 4) != TPS_E_CAPACITY || lcall(-1, 64, -64, 6, 4, -1, -4, -4) != TPS_E_CAPACITY) return 1;
    if (lcall(2, 64, 128, 0, 4, 2, 8, 8) != TPS_E_CAPACITY || lcall(2, 64, 128, 65, 4, 2, 8, 8) != TPS_E_CAPACITY) return 1;
    if (lcall(2, 64, 128, 6, 0, 2, 0, 0) != TPS_E_CAPACITY || lcall(2, 64, 128, 6, 257, 2, 514, 514) != TPS_E_CAPACITY) return 1;
    if (emu_sketch_links(nullptr, 0, 64, 0, 6, 4, nullptr, 0, nullptr, 0, nullptr, 0) != TPS_OK) return 1;
    printf("ok %d cases, %ld rows\n", n_cases, checked);
    return 0;
}
