// TEST INFRASTRUCTURE ONLY -- the placement emulation (emu_place.cpp) as a stand-alone program for the sanitizers:
//   g++ -fsanitize=address,undefined emu_place_main.cpp && ./a.out CASES
// CASES is a text file (tests/test_place.py writes the cases of tests/place_cases.py into it), one case after another:
//   pcase <k> <span> <max_occ> <n> <R>
//   <letters> <keep>                    n query lines, then R reference lines; keep is one 0 / 1 per letter; "-" is the empty window
// Every row is compared with a restatement of the rule below (strings, a map from k-mer to its entries, sorted vectors), so that the
// run also fails on a wrong answer, not only on a bad access.  Without an argument a small built-in batch runs.  Exit status 0 and
// "ok" = clean.
#include "emu_place.cpp"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

namespace {

int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'T' ? 2 : c == 'G' ? 3 : -1; }

struct Window { std::string letters; std::vector<char> keep; };     // keep[q] for every letter q

typedef std::map<std::string, std::vector<std::pair<int, int>>> Index;   // k-mer -> (r, q)

Index brute_index(const std::vector<Window>& refs, int k, int max_occ) {
    Index all, out;
    for (size_t r = 0; r < refs.size(); ++r)
        for (size_t q = 0; q + (size_t)k <= refs[r].letters.size(); ++q)
            if (refs[r].keep[q]) all[refs[r].letters.substr(q, (size_t)k)].push_back({(int)r, (int)q});
    for (auto& kv : all)
        if (kv.second.size() <= (size_t)max_occ) out.insert(kv);
    return out;
}

void brute_place(const Index& idx, int R, const Window& Q, int k, int32_t out[7]) {
    const int32_t none[7] = {-1, 0, -1, 0, 0, 0, 0};
    std::copy(none, none + 7, out);
    std::vector<int> total((size_t)R, 0);
    std::vector<std::pair<int, int>> hits;             // (r, d)
    for (size_t p = 0; p + (size_t)k <= Q.letters.size(); ++p) {
        if (!Q.keep[p]) continue;
        auto it = idx.find(Q.letters.substr(p, (size_t)k));
        if (it == idx.end()) continue;
        for (auto& e : it->second) { ++total[(size_t)e.first]; hits.push_back({e.first, e.second - (int)p}); }
    }
    if (hits.empty()) return;
    int ref = 0, run = -1;
    for (int r = 1; r < R; ++r)
        if (total[(size_t)r] > total[(size_t)ref]) ref = r;
    for (int r = 0; r < R; ++r)
        if (r != ref && total[(size_t)r] > 0 && (run < 0 || total[(size_t)r] > total[(size_t)run])) run = r;
    std::vector<int> ds;
    for (auto& h : hits)
        if (h.first == ref) ds.push_back(h.second);
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
    out[0] = ref; out[1] = total[(size_t)ref]; out[2] = run; out[3] = run < 0 ? 0 : total[(size_t)run];
    out[4] = fine[(fine.size() - 1) / 2]; out[5] = (int32_t)fine.size(); out[6] = second;
}

// the rows tps_batch_end_window writes
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

int check_place(const std::vector<Window>& qs, const std::vector<Window>& refs, int k, int span, int max_occ, long& checked) {
    std::vector<uint32_t> codes, keep, rcodes, rkeep;
    std::vector<int32_t> length, rlength;
    pack(qs, span, codes, keep, length);
    pack(refs, span, rcodes, rkeep, rlength);
    const int64_t n = (int64_t)qs.size();
    std::vector<int32_t> outs((size_t)(7 * n));
    const int rc = emu_window_place(codes.data(), (int64_t)codes.size(), keep.data(), (int64_t)keep.size(), length.data(), n, rcodes.data(), (int64_t)rcodes.size(),
                                    rkeep.data(), (int64_t)rkeep.size(), rlength.data(), (int)refs.size(), span, k, max_occ, outs.data(), n);
    if (rc != TPS_OK) { printf("place: rc %d (%s)\n", rc, emu_place_last_error()); return 1; }
    const Index idx = brute_index(refs, k, max_occ);
    for (int64_t i = 0; i < n; ++i) {
        int32_t want[7];
        brute_place(idx, (int)refs.size(), qs[(size_t)i], k, want);
        for (int j = 0; j < 7; ++j)
            if (outs[(size_t)(j * n + i)] != want[j]) {
                printf("k %d span %d max_occ %d, row %lld, output %d: got %d, want %d\n", k, span, max_occ, (long long)i, j, outs[(size_t)(j * n + i)], want[j]);
                return 1;
            }
        ++checked;
    }
    return 0;
}

bool read_window(std::istream& in, Window& w) {
    std::string line, bits;
    if (!std::getline(in, line)) return false;
    std::istringstream rl(line);
    if (!(rl >> w.letters >> bits)) return false;
    if (w.letters == "-") { w.letters.clear(); bits.clear(); }
    if (bits == "-") bits.clear();
    if (bits.size() != w.letters.size()) return false;
    for (char b : bits) w.keep.push_back(b == '1');
    return true;
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
            int k, span, max_occ;
            long n, R;
            if (!(hd >> tag >> k >> span >> max_occ >> n >> R) || tag != "pcase") { printf("bad case line: %s\n", line.c_str()); return 1; }
            std::vector<Window> qs((size_t)n), refs((size_t)R);
            for (Window& w : qs)
                if (!read_window(in, w)) { printf("bad window line\n"); return 1; }
            for (Window& w : refs)
                if (!read_window(in, w)) { printf("bad window line\n"); return 1; }
            if (check_place(qs, refs, k, span, max_occ, checked)) return 1;
            ++n_cases;
        }
    } else {
        uint32_t x = 8765;
        auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
        const int ks[] = {8, 12, 16};
        for (int k : ks) {
            const int span = k == 8 ? 1999 : k == 12 ? 4096 : 2001;
            std::vector<Window> refs, qs;
            std::string shared;                    // a piece every reference row holds: with max_occ 2 it takes no part
            for (int i = 0; i < 40; ++i) shared.push_back("ACGT"[rnd() & 3]);
            for (int r = 0; r < 5; ++r) {
                Window w;
                const int L = r == 3 ? 0 : span - 7 * r;
                for (int i = 0; i < L; ++i) w.letters.push_back("ACGT"[rnd() & 3]);
                if (L > 500) w.letters.replace(200, shared.size(), shared);
                for (int i = 0; i < L; ++i) w.keep.push_back(rnd() % 10u != 0);
                refs.push_back(w);
            }
            const int lens[] = {0, k - 1, k, 63 + k - 1, 64 + k - 1, 65 + k - 1, 500, span};
            for (int L : lens) {
                Window w;
                const Window& src = refs[(size_t)(rnd() % 3u)];
                const int from = (int)(rnd() % 300u);
                for (int i = 0; i < L; ++i) {
                    char c = from + i < (int)src.letters.size() ? src.letters[(size_t)(from + i)] : "ACGT"[rnd() & 3];
                    if (rnd() % 30u == 0) c = "ACGT"[rnd() & 3];
                    w.letters.push_back(c);
                    w.keep.push_back(rnd() % 8u != 0);
                }
                qs.push_back(w);
            }
            if (check_place(qs, refs, k, span, 16, checked) || check_place(qs, refs, k, span, 2, checked) || check_place(qs, refs, k, span, 64, checked)) return 1;
            ++n_cases;
        }
    }
    // the refusals, and an empty batch
    const uint32_t zc[21] = {0}, zk[12] = {0};
    int32_t o[14];
    auto call = [&](int64_t n, int R, int span, int k, int max_occ, int l0, int rl0, int64_t cl, int64_t kl, int64_t rcl, int64_t rkl, int64_t ol) {
        const int32_t len[2] = {l0, 5}, rlen[3] = {rl0, 0, 50};
        return emu_window_place(zc, cl, zk, kl, len, n, zc, rcl, zk, rkl, rlen, R, span, k, max_occ, o, ol);
    };
    if (call(2, 3, 100, 12, 16, 100, 100, 14, 8, 21, 12, 2) != TPS_OK || o[0] != -1 || o[2] != 0 || o[4] != -1 || o[13] != 0) return 1;
    if (call(262145, 3, 100, 12, 16, 100, 100, 262145 * 7, 262145 * 4, 21, 12, 262145) != TPS_E_CAPACITY || call(-1, 3, 100, 12, 16, 100, 100, -7, -4, 21, 12, -1) != TPS_E_CAPACITY) return 1;
    if (call(2, 0, 100, 12, 16, 100, 100, 14, 8, 0, 0, 2) != TPS_E_CAPACITY || call(2, 1025, 100, 12, 16, 100, 100, 14, 8, 1025 * 7, 1025 * 4, 2) != TPS_E_CAPACITY) return 1;
    if (call(2, 3, 11, 12, 16, 5, 5, 2, 2, 3, 3, 2) != TPS_E_CAPACITY || call(2, 3, 4097, 12, 16, 100, 100, 514, 258, 771, 387, 2) != TPS_E_CAPACITY) return 1;
    if (call(2, 3, 100, 7, 16, 100, 100, 14, 8, 21, 12, 2) != TPS_E_CAPACITY || call(2, 3, 100, 17, 16, 100, 100, 14, 8, 21, 12, 2) != TPS_E_CAPACITY) return 1;
    if (call(2, 3, 100, 12, 0, 100, 100, 14, 8, 21, 12, 2) != TPS_E_CAPACITY || call(2, 3, 100, 12, 65, 100, 100, 14, 8, 21, 12, 2) != TPS_E_CAPACITY) return 1;
    if (call(2, 3, 100, 12, 16, 101, 100, 14, 8, 21, 12, 2) != TPS_E_ARG || call(2, 3, 100, 12, 16, -1, 100, 14, 8, 21, 12, 2) != TPS_E_ARG) return 1;
    if (call(2, 3, 100, 12, 16, 100, 101, 14, 8, 21, 12, 2) != TPS_E_ARG || call(2, 3, 100, 12, 16, 100, -1, 14, 8, 21, 12, 2) != TPS_E_ARG) return 1;
    if (call(2, 3, 100, 12, 16, 100, 100, 13, 8, 21, 12, 2) != TPS_E_ARG || call(2, 3, 100, 12, 16, 100, 100, 14, 9, 21, 12, 2) != TPS_E_ARG) return 1;
    if (call(2, 3, 100, 12, 16, 100, 100, 14, 8, 20, 12, 2) != TPS_E_ARG || call(2, 3, 100, 12, 16, 100, 100, 14, 8, 21, 11, 2) != TPS_E_ARG || call(2, 3, 100, 12, 16, 100, 100, 14, 8, 21, 12, 1) != TPS_E_ARG) return 1;
    if (call(0, 3, 100, 12, 16, 100, 100, 0, 0, 21, 12, 0) != TPS_OK) return 1;
    printf("ok %d cases, %ld rows\n", n_cases, checked);
    return 0;
}
