// TEST INFRASTRUCTURE ONLY -- the window and offset emulation (emu_anchor.cpp) as a stand-alone program for the sanitizers:
//   g++ -fsanitize=address,undefined emu_anchor_main.cpp && ./a.out CASES
// CASES is a text file (tests/test_anchor.py writes the cases of tests/anchor_cases.py into it), one case after another:
//   wcase <unit> <k> <span> <n>         reads and windows: extracted, then set against each other
//   <tail> <begin> <end> <ref> <read>   n lines; "-" is the empty read
//   ocase <k> <span> <n>                windows by hand
//   <ref> <letters> <keep>              n lines; keep is one 0 / 1 per letter; "-" is the empty window
// Every row is compared with a position-by-position restatement of the two rules below (strings, a map, a sorted vector), so that
// the run also fails on a wrong answer, not only on a bad access.  Without an argument a small built-in batch runs.  Exit status 0
// and "ok" = clean.
#include "emu_anchor.cpp"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
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

struct Read { std::string seq; int tail, begin, end, ref; };
struct Window { std::string letters; std::vector<char> keep; int ref; };     // keep[q] for every letter q

Window brute_window(const Read& rd, const std::string& unit, int k) {
    const int w = std::min((int)unit.size(), 8);
    std::string h;
    for (char c : rd.seq) h.push_back((char)(c >= 'a' && c <= 'z' ? c - 32 : c));
    if (rd.tail) h = revcomp(h);
    const std::string rc = revcomp(unit);
    const long e = std::min((long)rd.end, (long)h.size());
    Window out;
    out.ref = rd.ref;
    if (e > rd.begin) out.letters = h.substr((size_t)rd.begin, (size_t)(e - rd.begin));
    out.keep.assign(out.letters.size(), 0);
    for (long i = rd.begin; i + k <= e; ++i) {
        bool ok = true;
        for (int q = 0; q < k && ok; ++q) ok = code_of(h[(size_t)(i + q)]) >= 0;
        for (int d = 0; d <= k - w && ok; ++d)
            if (near(h, (size_t)(i + d), unit, w) || near(h, (size_t)(i + d), rc, w)) ok = false;
        out.keep[(size_t)(i - rd.begin)] = ok;
    }
    return out;
}

uint32_t kmer_hash(const std::string& s, size_t at, int k) {
    uint32_t c = 0;
    for (int q = 0; q < k; ++q) c |= (uint32_t)std::max(code_of(s[at + (size_t)q]), 0) << (2 * q);
    return fmix(c ^ 0x9E3779B9u);
}

void brute_offset(const Window& R, const Window& Q, int k, int32_t out[3]) {
    std::map<uint32_t, std::pair<uint32_t, int>> table;
    for (size_t q = 0; q + (size_t)k <= R.letters.size(); ++q) {
        if (!R.keep[q]) continue;
        const uint32_t x = kmer_hash(R.letters, q, k);
        const std::pair<uint32_t, int> cand(x & 0xFFFFFu, (int)q);
        auto it = table.find(x >> 20);
        if (it == table.end() || cand < it->second) table[x >> 20] = cand;
    }
    std::vector<int> ds;
    for (size_t p = 0; p + (size_t)k <= Q.letters.size(); ++p) {
        if (!Q.keep[p]) continue;
        const uint32_t x = kmer_hash(Q.letters, p, k);
        auto it = table.find(x >> 20);
        if (it != table.end() && it->second.first == (x & 0xFFFFFu)) ds.push_back(it->second.second - (int)p);
    }
    std::sort(ds.begin(), ds.end());
    int H[129] = {0};
    for (int d : ds) ++H[(d + 4096) / 64];
    int best = 0, top = -1, second = 0;
    for (int c = 0; c < 127; ++c)
        if (H[c] + H[c + 1] > top) { top = H[c] + H[c + 1]; best = c; }
    for (int c = 0; c < 127; ++c)
        if (std::abs(c - best) >= 2) second = std::max(second, H[c] + H[c + 1]);
    std::vector<int> fine;
    for (int d : ds)
        if (d >= 64 * best - 4096 && d < 64 * best - 3968) fine.push_back(d);
    out[0] = fine.empty() ? 0 : fine[(fine.size() - 1) / 2];
    out[1] = (int32_t)fine.size();
    out[2] = second;
}

// the rows tps_batch_end_window writes, from the brute windows
void pack(const std::vector<Window>& ws, int span, std::vector<uint32_t>& codes, std::vector<uint32_t>& keep, std::vector<int32_t>& length) {
    const int cdw = (span + 15) / 16, kdw = (span + 31) / 32;
    codes.assign(ws.size() * (size_t)cdw, 0);
    keep.assign(ws.size() * (size_t)kdw, 0);
    length.clear();
    for (size_t r = 0; r < ws.size(); ++r) {
        for (size_t q = 0; q < ws[r].letters.size(); ++q) {
            codes[r * (size_t)cdw + (q >> 4)] |= (uint32_t)std::max(code_of(ws[r].letters[q]), 0) << (2 * (q & 15));
            if (ws[r].keep[q]) keep[r * (size_t)kdw + (q >> 5)] |= 1u << (q & 31);
        }
        length.push_back((int32_t)ws[r].letters.size());
    }
}

int check_offsets(const std::vector<Window>& ws, int k, int span, long& checked) {
    std::vector<uint32_t> codes, keep;
    std::vector<int32_t> length, ref;
    pack(ws, span, codes, keep, length);
    for (const Window& w : ws) ref.push_back(w.ref);
    const int64_t n = (int64_t)ws.size();
    std::vector<int32_t> off((size_t)n), votes((size_t)n), second((size_t)n);
    const int rc = emu_window_offsets(codes.data(), keep.data(), length.data(), ref.data(), n, span, k, off.data(), votes.data(), second.data(), n);
    if (rc != TPS_OK) { printf("offsets: rc %d (%s)\n", rc, emu_anchor_last_error()); return 1; }
    for (int64_t i = 0; i < n; ++i) {
        int32_t want[3] = {0, 0, 0};
        if (ref[(size_t)i] >= 0) brute_offset(ws[(size_t)ref[(size_t)i]], ws[(size_t)i], k, want);
        if (off[(size_t)i] != want[0] || votes[(size_t)i] != want[1] || second[(size_t)i] != want[2]) {
            printf("k %d span %d, row %lld: got %d %d %d, want %d %d %d\n", k, span, (long long)i, off[(size_t)i], votes[(size_t)i], second[(size_t)i], want[0], want[1], want[2]);
            return 1;
        }
        ++checked;
    }
    return 0;
}

int run_wcase(const std::string& unit, int k, int span, const std::vector<Read>& reads, int shift, long& checked) {
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
    const int cdw = (span + 15) / 16, kdw = (span + 31) / 32;
    std::vector<uint32_t> codes((size_t)(n * cdw)), keep((size_t)(n * kdw));
    const int rc = emu_end_window(bases.data(), offsets.data(), n, code_unit(unit), (int)unit.size(), k, tails.data(), begin.data(), end.data(), n, span, shift,
                                  codes.data(), n * cdw, keep.data(), n * kdw);
    if (rc != TPS_OK) { printf("unit %s: rc %d (%s)\n", unit.c_str(), rc, emu_anchor_last_error()); return 1; }
    std::vector<Window> ws;
    for (const Read& r : reads) ws.push_back(brute_window(r, unit, k));
    std::vector<uint32_t> wc, wk;
    std::vector<int32_t> wl;
    pack(ws, span, wc, wk, wl);
    if (wc != codes || wk != keep) {
        for (int64_t r = 0; r < n; ++r)
            if (!std::equal(wc.begin() + r * cdw, wc.begin() + (r + 1) * cdw, codes.begin() + r * cdw) || !std::equal(wk.begin() + r * kdw, wk.begin() + (r + 1) * kdw, keep.begin() + r * kdw)) {
                printf("unit %s k %d span %d: the window of read %lld differs\n", unit.c_str(), k, span, (long long)r);
                return 1;
            }
    }
    checked += (long)n;
    return check_offsets(ws, k, span, checked);
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
            int k, span;
            long n;
            hd >> tag;
            if (tag == "wcase" && (hd >> unit >> k >> span >> n)) {
                std::vector<Read> reads;
                for (long i = 0; i < n; ++i) {
                    if (!std::getline(in, line)) { printf("the file ends inside a case\n"); return 1; }
                    std::istringstream rl(line);
                    Read r;
                    if (!(rl >> r.tail >> r.begin >> r.end >> r.ref >> r.seq)) { printf("bad read line\n"); return 1; }
                    if (r.seq == "-") r.seq.clear();
                    reads.push_back(r);
                }
                if (run_wcase(unit, k, span, reads, n_cases & 3, checked)) return 1;
            } else if (tag == "ocase" && (hd >> k >> span >> n)) {
                std::vector<Window> ws;
                for (long i = 0; i < n; ++i) {
                    if (!std::getline(in, line)) { printf("the file ends inside a case\n"); return 1; }
                    std::istringstream rl(line);
                    Window w;
                    std::string bits;
                    if (!(rl >> w.ref >> w.letters >> bits)) { printf("bad window line\n"); return 1; }
                    if (w.letters == "-") { w.letters.clear(); bits.clear(); }
                    if (bits.size() != w.letters.size()) { printf("keep and letters differ in length\n"); return 1; }
                    for (char b : bits) w.keep.push_back(b == '1');
                    ws.push_back(w);
                }
                if (check_offsets(ws, k, span, checked)) return 1;
            } else {
                printf("bad case line: %s\n", line.c_str());
                return 1;
            }
            ++n_cases;
        }
    } else {
        uint32_t x = 4321;
        auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
        const std::string units[] = {"AAAC", "CCCTAA", "CTGTGGGGTCTGGGTG", "ACGGTTCAGTCCATGACTTGCAAGTCTGATCC"};
        for (const std::string& unit : units) {
            std::string sub;                       // one subtelomere shared by the reads: their windows vote for each other
            for (int i = 0; i < 9000; ++i) sub.push_back("ACGT"[rnd() & 3]);
            const int lens[] = {0, 3, 11, 12, 13, 75, 76, 500, 4210, 4300, 4346, 9000};
            const int n_lens = (int)(sizeof lens / sizeof lens[0]);
            std::vector<Read> reads;
            for (int L : lens) {
                std::string r;
                for (int i = 0; i < L; ++i) {
                    char c = i < 300 ? unit[(size_t)i % unit.size()] : sub[(size_t)i];
                    if (rnd() % 500u == 0) c = 'N';
                    if (rnd() % 40u == 0) c = "ACGT"[rnd() & 3];
                    r.push_back(c);
                }
                const int tail = (int)(rnd() & 1);
                const int b = L > 400 ? 250 + (int)(rnd() % 60u) : 0;
                reads.push_back(Read{tail ? revcomp(r) : r, tail, b, b + 4096, (int)(rnd() % (unsigned)n_lens)});
            }
            reads[0].ref = -1;
            reads[n_lens - 1].ref = n_lens - 1;
            if (run_wcase(unit, 12, 4096, reads, n_cases & 3, checked)) return 1;
            for (Read& r : reads) r.end = r.begin + 1999;
            if (run_wcase(unit, 8, 1999, reads, n_cases & 3, checked) || run_wcase(unit, 16, 2001, reads, n_cases & 3, checked)) return 1;
            ++n_cases;
        }
    }
    // the refusals, and an empty batch
    const uint8_t one_read[4] = {'A', 'C', 'G', 'T'};
    const int64_t off[2] = {0, 3};
    uint32_t co[256], kp[128];
    const uint64_t u6 = code_unit("CCCTAA");
    auto call = [&](uint64_t unit, int m, int k, int span, int tail, int b, int e, int64_t nr, int64_t cl, int64_t kl) {
        const uint8_t t[1] = {(uint8_t)tail};
        const int32_t bb[1] = {b}, ee[1] = {e};
        return emu_end_window(one_read, off, 1, unit, m, k, t, bb, ee, nr, span, 0, co, cl, kp, kl);
    };
    if (call(u6, 6, 12, 100, 0, 0, 3, 1, 7, 4) != TPS_OK || co[0] != (0u | 1u << 2 | 3u << 4) || co[6] != 0 || kp[0] != 0 || kp[3] != 0) return 1;
    if (call(u6, 3, 12, 100, 0, 0, 3, 1, 7, 4) != TPS_E_ARG || call(code_unit("CCACCA"), 6, 12, 100, 0, 0, 3, 1, 7, 4) != TPS_E_ARG) return 1;
    if (call(u6, 6, 7, 100, 0, 0, 3, 1, 7, 4) != TPS_E_CAPACITY || call(u6, 6, 17, 100, 0, 0, 3, 1, 7, 4) != TPS_E_CAPACITY) return 1;
    if (call(u6, 6, 12, 11, 0, 0, 3, 1, 1, 1) != TPS_E_CAPACITY || call(u6, 6, 12, 4097, 0, 0, 3, 1, 257, 129) != TPS_E_CAPACITY) return 1;
    if (call(u6, 6, 12, 100, 2, 0, 3, 1, 7, 4) != TPS_E_ARG || call(u6, 6, 12, 100, 0, -1, 3, 1, 7, 4) != TPS_E_ARG || call(u6, 6, 12, 100, 0, 4, 3, 1, 7, 4) != TPS_E_ARG) return 1;
    if (call(u6, 6, 12, 100, 0, 0, 101, 1, 7, 4) != TPS_E_CAPACITY || call(u6, 6, 12, 100, 0, 0, 100, 1, 7, 4) != TPS_OK) return 1;
    if (call(u6, 6, 12, 4096, 0, 0, 16385, 1, 256, 128) != TPS_E_CAPACITY || call(u6, 6, 12, 4096, 0, 0, 4096, 1, 256, 128) != TPS_OK) return 1;
    if (call(u6, 6, 12, 100, 0, 0, 3, 2, 7, 4) != TPS_E_ARG || call(u6, 6, 12, 100, 0, 0, 3, 1, 6, 4) != TPS_E_ARG || call(u6, 6, 12, 100, 0, 0, 3, 1, 7, 3) != TPS_E_ARG) return 1;
    if (emu_end_window(one_read, off, 0, u6, 6, 12, nullptr, nullptr, nullptr, 0, 100, 0, nullptr, 0, nullptr, 0) != TPS_OK) return 1;
    int32_t o3[6];
    const uint32_t zc[14] = {0}, zk[8] = {0};
    auto ocall = [&](int64_t n, int span, int k, int l0, int r0, int64_t ol) {
        const int32_t len[2] = {l0, 5}, ref[2] = {r0, -7};
        return emu_window_offsets(zc, zk, len, ref, n, span, k, o3, o3 + 2, o3 + 4, ol);
    };
    if (ocall(2, 100, 12, 100, 1, 2) != TPS_OK || o3[0] != 0 || o3[2] != 0 || o3[5] != 0) return 1;
    if (ocall(262145, 100, 12, 100, 1, 262145) != TPS_E_CAPACITY || ocall(-1, 100, 12, 100, 1, -1) != TPS_E_CAPACITY) return 1;
    if (ocall(2, 11, 12, 5, 1, 2) != TPS_E_CAPACITY || ocall(2, 4097, 12, 100, 1, 2) != TPS_E_CAPACITY) return 1;
    if (ocall(2, 100, 7, 100, 1, 2) != TPS_E_CAPACITY || ocall(2, 100, 17, 100, 1, 2) != TPS_E_CAPACITY) return 1;
    if (ocall(2, 100, 12, 100, 2, 2) != TPS_E_ARG || ocall(2, 100, 12, 101, 1, 2) != TPS_E_ARG || ocall(2, 100, 12, -1, 1, 2) != TPS_E_ARG || ocall(2, 100, 12, 100, 1, 1) != TPS_E_ARG) return 1;
    if (emu_window_offsets(nullptr, nullptr, nullptr, nullptr, 0, 100, 12, nullptr, nullptr, nullptr, 0) != TPS_OK) return 1;
    printf("ok %d cases, %ld rows\n", n_cases, checked);
    return 0;
}
