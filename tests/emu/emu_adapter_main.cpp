// TEST INFRASTRUCTURE ONLY -- the adapter emulation (emu_adapter.cpp) as a stand-alone program for the sanitizers:
//   g++ -fsanitize=address,undefined emu_adapter_main.cpp && ./a.out CASES
// CASES is a text file (tests/test_adapter.py writes the cases of tests/adapter_cases.py into it), one case after another:
//   acase <n_pat> <n_reads>
//   <pattern>                       n_pat lines
//   <tail> <begin> <end> <read>     n_reads lines; "-" is the empty read
// Every answer is compared with the plain two-row dynamic programme below (strings, no bit vectors), so that the run also fails on a
// wrong answer, not only on a bad access.  The staging area is one wave's, poisoned, and every row has exactly its size
// (emu_adapter_find).  Without an argument a small built-in batch runs.  Exit status 0 and "ok" = clean.
#include "emu_adapter.cpp"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

namespace {

int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'T' ? 2 : c == 'G' ? 3 : -1; }

std::string revcomp(const std::string& u) {
    std::string t(u.rbegin(), u.rend());
    for (char& c : t) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
    return t;
}

struct Read { std::string seq; int tail, begin, end; };

// (dist, end) of pattern p in the region of rd: Sellers' recurrence, row by row of the text
void brute(const Read& rd, const std::string& p, int out[2]) {
    std::string h;
    for (char c : rd.seq) h.push_back((char)(c >= 'a' && c <= 'z' ? c - 32 : c));
    if (rd.tail) h = revcomp(h);
    const long e = std::min((long)rd.end, (long)h.size());
    const std::string T = e > rd.begin ? h.substr((size_t)rd.begin, (size_t)(e - rd.begin)) : std::string();
    const int m = (int)p.size();
    std::vector<int> col((size_t)m + 1), nxt((size_t)m + 1);
    for (int i = 0; i <= m; ++i) col[(size_t)i] = i;
    out[0] = m; out[1] = 0;
    for (size_t t = 0; t < T.size(); ++t) {
        nxt[0] = 0;
        for (int i = 1; i <= m; ++i) {
            const int sub = col[(size_t)i - 1] + ((code_of(T[t]) >= 0 && T[t] == p[(size_t)i - 1]) ? 0 : 1);
            nxt[(size_t)i] = std::min(sub, std::min(col[(size_t)i] + 1, nxt[(size_t)i - 1] + 1));
        }
        col.swap(nxt);
        if (col[(size_t)m] < out[0]) { out[0] = col[(size_t)m]; out[1] = (int)t + 1; }
    }
}

void code_patterns(const std::vector<std::string>& pats, std::vector<uint64_t>& codes, std::vector<int32_t>& lens) {
    codes.assign(pats.size() * 2, 0);
    lens.clear();
    for (size_t j = 0; j < pats.size(); ++j) {
        for (size_t i = 0; i < pats[j].size() && i < 64; ++i) codes[2 * j + (i >> 5)] |= (uint64_t)code_of(pats[j][i]) << (2 * (i & 31));
        lens.push_back((int32_t)pats[j].size());
    }
}

int run_case(const std::vector<std::string>& pats, const std::vector<Read>& reads, int shift, long& checked) {
    std::vector<uint8_t> bases, tails;
    std::vector<int64_t> offsets{0};
    std::vector<int32_t> begin, end;
    for (const Read& r : reads) {
        bases.insert(bases.end(), r.seq.begin(), r.seq.end());
        offsets.push_back((int64_t)bases.size());
        tails.push_back((uint8_t)r.tail); begin.push_back(r.begin); end.push_back(r.end);
    }
    bases.push_back(0);
    std::vector<uint64_t> codes;
    std::vector<int32_t> lens;
    code_patterns(pats, codes, lens);
    const int64_t n = (int64_t)reads.size();
    const int P = (int)pats.size();
    std::vector<uint16_t> hits((size_t)(n * P * 2));           // exactly the rows
    const int rc = emu_adapter_find(bases.data(), offsets.data(), n, codes.data(), lens.data(), P, tails.data(), begin.data(), end.data(), n, shift,
                                    hits.data(), n * P * 2);
    if (rc != TPS_OK) { printf("rc %d (%s)\n", rc, emu_adapter_last_error()); return 1; }
    for (int64_t r = 0; r < n; ++r)
        for (int j = 0; j < P; ++j) {
            int want[2];
            brute(reads[(size_t)r], pats[(size_t)j], want);
            const uint16_t* got = &hits[(size_t)((r * P + j) * 2)];
            if (got[0] != want[0] || got[1] != want[1]) {
                printf("read %lld pattern %d: got (%d, %d), want (%d, %d)\n", (long long)r, j, got[0], got[1], want[0], want[1]);
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
            std::string tag;
            long P, n;
            if (!(hd >> tag >> P >> n) || tag != "acase") { printf("bad case line: %s\n", line.c_str()); return 1; }
            std::vector<std::string> pats;
            std::vector<Read> reads;
            for (long j = 0; j < P; ++j) {
                if (!std::getline(in, line)) { printf("the file ends inside a case\n"); return 1; }
                pats.push_back(line);
            }
            for (long i = 0; i < n; ++i) {
                if (!std::getline(in, line)) { printf("the file ends inside a case\n"); return 1; }
                std::istringstream rl(line);
                Read r;
                if (!(rl >> r.tail >> r.begin >> r.end >> r.seq)) { printf("bad read line\n"); return 1; }
                if (r.seq == "-") r.seq.clear();
                reads.push_back(r);
            }
            if (run_case(pats, reads, n_cases & 3, checked)) return 1;
            ++n_cases;
        }
    } else {
        uint32_t x = 8765;
        auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
        auto word = [&](int len) { std::string s; for (int i = 0; i < len; ++i) s.push_back("ACGT"[rnd() & 3]); return s; };
        const int pcounts[] = {1, 2, 63, 64};
        for (int P : pcounts) {
            std::vector<std::string> pats;
            const int mlens[] = {12, 31, 32, 33, 63, 64, 24, 40};
            for (int j = 0; j < P; ++j) pats.push_back(word(mlens[j % 8]));
            pats[0] = std::string(64, 'A');
            std::vector<Read> reads;
            const int lens[] = {0, 1, 11, 12, 63, 64, 65, 255, 256, 257, 1024, 1500, 3000};
            for (int L : lens) {
                std::string r = word(L);
                // an occurrence of some pattern with a few errors, somewhere in the first bases
                const std::string& p = pats[rnd() % (unsigned)P];
                const int at = L > 80 ? (int)(rnd() % 40u) : 0;
                for (size_t i = 0; i < p.size() && at + (int)i < L; ++i) r[(size_t)at + i] = rnd() % 12u == 0 ? 'N' : p[i];
                if (L == 1500) r = std::string(100, 'A') + r.substr(100);
                const int tail = (int)(rnd() & 1);
                const int b = (int)(rnd() % 17u);
                std::string s = tail ? revcomp(r) : r;
                if (L == 255) for (char& c : s) c = (char)(c + 32);            // lower case
                reads.push_back(Read{s, tail, b, b + 1 + (int)(rnd() % 1024u)});
            }
            reads.push_back(Read{word(2000), 1, 5, 1029});
            reads.push_back(Read{word(300), 0, 400, 500});
            if (run_case(pats, reads, n_cases & 3, checked)) return 1;
            ++n_cases;
        }
    }
    // the refusals, and an empty batch
    const uint8_t one_read[4] = {'A', 'C', 'G', 'T'};
    const int64_t off[2] = {0, 3};
    uint16_t hit[4];
    auto call = [&](uint64_t lo, uint64_t hi, int m, int P, int tail, int b, int e, int64_t nr, int64_t hl) {
        const uint64_t pat[4] = {lo, hi, lo, hi};
        const int32_t len[2] = {m, m};
        const uint8_t t[1] = {(uint8_t)tail};
        const int32_t bb[1] = {b}, ee[1] = {e};
        return emu_adapter_find(one_read, off, 1, pat, len, P, t, bb, ee, nr, 0, hit, hl);
    };
    if (call(0, 0, 12, 1, 0, 0, 3, 1, 2) != TPS_OK || hit[0] != 11 || hit[1] != 1) return 1;      // A x 12 against "ACG": the A, 11 letters missing
    if (call(0, 0, 12, 0, 0, 0, 3, 1, 0) != TPS_E_CAPACITY || call(0, 0, 12, 65, 0, 0, 3, 1, 130) != TPS_E_CAPACITY) return 1;
    if (call(0, 0, 11, 1, 0, 0, 3, 1, 2) != TPS_E_CAPACITY || call(0, 0, 65, 1, 0, 0, 3, 1, 2) != TPS_E_CAPACITY) return 1;
    if (call(1ull << 24, 0, 12, 1, 0, 0, 3, 1, 2) != TPS_E_ARG || call(0, 1, 32, 1, 0, 0, 3, 1, 2) != TPS_E_ARG || call(0, 1ull << 2, 33, 1, 0, 0, 3, 1, 2) != TPS_E_ARG) return 1;
    if (call(~0ull, ~0ull, 64, 1, 0, 0, 3, 1, 2) != TPS_OK || call(~0ull, 3, 33, 1, 0, 0, 3, 1, 2) != TPS_OK) return 1;
    if (call(0, 0, 12, 1, 2, 0, 3, 1, 2) != TPS_E_ARG || call(0, 0, 12, 1, 0, -1, 3, 1, 2) != TPS_E_ARG || call(0, 0, 12, 1, 0, 4, 3, 1, 2) != TPS_E_ARG) return 1;
    if (call(0, 0, 12, 1, 0, 0, 1025, 1, 2) != TPS_E_CAPACITY || call(0, 0, 12, 1, 0, 0, 1024, 1, 2) != TPS_OK) return 1;
    if (call(0, 0, 12, 1, 0, 0, 3, 2, 2) != TPS_E_ARG || call(0, 0, 12, 1, 0, 0, 3, 1, 1) != TPS_E_ARG || call(0, 0, 12, 2, 0, 0, 3, 1, 2) != TPS_E_ARG) return 1;
    const uint64_t p0[2] = {0, 0};
    const int32_t l0[1] = {12};
    if (emu_adapter_find(one_read, off, 0, p0, l0, 1, nullptr, nullptr, nullptr, 0, 0, nullptr, 0) != TPS_OK) return 1;
    printf("ok %d cases, %ld answers\n", n_cases, checked);
    return 0;
}
