// TEST INFRASTRUCTURE ONLY -- the motif census emulation (emu_motif.cpp) as a stand-alone program for the sanitizers:
//   g++ -fsanitize=address,undefined emu_motif_main.cpp && ./a.out
// A few of the edge cases of tests/motif_cases.py are built in; every answer is compared with a position-by-position restatement
// of the rule below, so that the run also fails on a wrong answer, not only on a bad access.  Exit status 0 and "ok" = clean.
#include "emu_motif.cpp"

#include <algorithm>
#include <cstdio>

namespace {

struct Want { uint64_t unit; int period, support, run_start, run_len, n_bases; std::vector<int> c; };

bool acgt(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

Want brute(const std::string& read, int e, int u_min, int u_max, int lo, int hi, int min_len) {
    Want w{0, 0, 0, 0, 0, 0, std::vector<int>((size_t)(u_max - u_min + 1), 0)};
    if ((int)read.size() <= min_len) return w;
    std::string s;
    for (char c : read) s.push_back((char)(c >= 'a' && c <= 'z' ? c - 32 : c));
    if (e) {
        std::string t(s.rbegin(), s.rend());
        for (char& c : t) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
        s = t;
    }
    const std::string h = (int)s.size() > lo ? s.substr((size_t)lo, (size_t)(std::min((int)s.size(), hi) - lo)) : std::string();
    const int n = (int)h.size();
    int best_u = 0, best_c = 0, best_s = 0, best_l = 0;
    for (int u = u_min; u <= u_max; ++u) {
        const int wd = u < 8 ? u : 8;
        int c = 0, run = 0, rs = 0, rl = 0;
        for (int i = 0; i < n; ++i) {
            bool per = i + u + wd <= n;
            for (int t = 0; per && t < wd; ++t) per = acgt(h[(size_t)(i + t)]) && h[(size_t)(i + t)] == h[(size_t)(i + t + u)];
            run = per ? run + 1 : 0;
            c += per;
            if (run > rl) { rl = run; rs = i - run + 1; }
        }
        w.c[(size_t)(u - u_min)] = c;
        if (c > best_c) { best_c = c; best_u = u; best_s = rs; best_l = rl; }
    }
    if (!best_c) return w;
    for (int j = 0; j < best_u; ++j) {
        const char c = h[(size_t)(best_s + j)];
        const uint64_t v = acgt(c) ? (c == 'A' ? 0 : c == 'C' ? 1 : c == 'T' ? 2 : 3) : (uint64_t)((((unsigned char)c >> 1) & 3) ^ (e ? 2 : 0));
        w.unit |= v << (2 * j);
    }
    w.period = best_u; w.support = best_c; w.run_start = best_s; w.run_len = best_l; w.n_bases = n;
    return w;
}

}  // namespace

int main() {
    std::string tract, m32 = "ACGGTTCAGTCCATGACTTGCAAGTCTGATCC", rnd;
    for (int i = 0; i < 1000; ++i) tract += "CCCTAA";
    uint32_t x = 12345;
    for (int i = 0; i < 3000; ++i) { x = x * 1664525u + 1013904223u; rnd.push_back("ACGT"[x >> 30]); }
    std::string n_run = tract.substr(0, 240) + "N" + tract.substr(0, 240) + "RYK" + tract.substr(0, 360) + rnd.substr(0, 700);
    std::string m32s;
    for (int i = 0; i < 150; ++i) m32s += m32;
    std::vector<std::string> reads = {tract, std::string(5000, 'A'), n_run, m32s, m32.substr(0, 20) + "N" + m32.substr(21) + m32.substr(0, 19),
                                      rnd, rnd.substr(0, 700), tract.substr(0, 360) + rnd.substr(0, 100), std::string(300, 'N'),
                                      "", "A", "AC", tract.substr(0, 11), tract.substr(0, 12), tract.substr(0, 15), tract.substr(0, 16), tract.substr(0, 17),
                                      tract.substr(0, 31), tract.substr(0, 32), tract.substr(0, 33), tract.substr(0, 63), tract.substr(0, 64), tract.substr(0, 65)};
    for (auto& c : reads[7]) c = (char)(c + 32);                     // a lower-case read
    std::vector<uint8_t> bases;
    std::vector<int64_t> offsets{0};
    for (const std::string& r : reads) {
        bases.insert(bases.end(), r.begin(), r.end());
        offsets.push_back((int64_t)bases.size());
    }
    bases.push_back(0);                                               // (a valid pointer for an all-empty batch)
    const int64_t n = (int64_t)reads.size();
    // u_min, u_max, lo, hi, min_len
    const int prm[][5] = {{4, 32, 0, 1000, 0}, {1, 32, 7, 4103, 0}, {4, 32, 0, 4096, 0}, {32, 32, 0, 2000, 0}, {1, 1, 0, 1000, 0}, {6, 6, 0, 11, 0},
                          {6, 6, 0, 12, 0}, {12, 12, 5, 24, 0}, {12, 12, 5, 25, 0}, {32, 32, 0, 39, 0}, {32, 32, 0, 40, 0}, {1, 4, 10, 11, 0},
                          {1, 32, 0, 31, 0}, {1, 32, 0, 32, 0}, {1, 32, 0, 33, 0}, {4, 32, 61, 125, 0}, {4, 32, 0, 1000, 360}};
    int checked = 0;
    for (size_t p = 0; p < sizeof(prm) / sizeof(prm[0]); ++p) {
        const int u_min = prm[p][0], u_max = prm[p][1], lo = prm[p][2], hi = prm[p][3], min_len = prm[p][4], nu = u_max - u_min + 1;
        std::vector<tps_motif_hit> hits((size_t)(2 * n));
        std::vector<int32_t> counts((size_t)(2 * n * nu));
        const int rc = emu_motif_census(bases.data(), offsets.data(), n, u_min, u_max, lo, hi, min_len, (int)(p & 3), hits.data(), 2 * n, counts.data(), 2 * n * nu);
        if (rc != TPS_OK) { printf("parameter set %zu: rc %d (%s)\n", p, rc, emu_motif_last_error()); return 1; }
        for (int64_t r = 0; r < n; ++r)
            for (int e = 0; e < 2; ++e) {
                const Want w = brute(reads[(size_t)r], e, u_min, u_max, lo, hi, min_len);
                const tps_motif_hit& g = hits[(size_t)(2 * r + e)];
                bool ok = g.unit == w.unit && g.period == w.period && g.support == w.support && g.run_start == w.run_start && g.run_len == w.run_len &&
                          g.n_bases == w.n_bases && g.reserved == 0;
                for (int i = 0; i < nu; ++i) ok = ok && counts[(size_t)((2 * r + e) * nu + i)] == w.c[(size_t)i];
                if (!ok) {
                    printf("parameter set %zu, read %lld, end %d: got period %d support %d run %d+%d unit %llx n %d, want period %d support %d run %d+%d unit %llx n %d\n",
                           p, (long long)r, e, g.period, g.support, g.run_start, g.run_len, (unsigned long long)g.unit, g.n_bases, w.period, w.support,
                           w.run_start, w.run_len, (unsigned long long)w.unit, w.n_bases);
                    return 1;
                }
                ++checked;
            }
    }
    // the refusals, and an empty batch
    tps_motif_hit one[2];
    if (emu_motif_census(bases.data(), offsets.data(), 1, 0, 4, 0, 100, 0, 0, one, 2, nullptr, 0) != TPS_E_ARG) return 1;
    if (emu_motif_census(bases.data(), offsets.data(), 1, 4, 33, 0, 100, 0, 0, one, 2, nullptr, 0) != TPS_E_ARG) return 1;
    if (emu_motif_census(bases.data(), offsets.data(), 1, 4, 32, 0, 4097, 0, 0, one, 2, nullptr, 0) != TPS_E_CAPACITY) return 1;
    if (emu_motif_census(bases.data(), offsets.data(), 0, 4, 32, 0, 1000, 0, 0, nullptr, 0, nullptr, 0) != TPS_OK) return 1;
    printf("ok %d read ends\n", checked);
    return 0;
}
