// TEST INFRASTRUCTURE ONLY -- the banded alignment emulation (emu_align.cpp) as a stand-alone program for the sanitizers:
//   g++ -fsanitize=address,undefined emu_align_main.cpp && ./a.out CASES
// CASES is a text file (tests/test_align.py writes the cases of tests/align_cases.py into it), one case after another:
//   acase <span> <n_ref> <n> <n_pile>
//   <letters>                                 n_ref lines; "-" is the empty window
//   <ref> <centre> <pile_row> <letters>       n lines
// Every pair is compared with a cell-by-cell restatement of the rule below (strings, the full table, no lanes), so that the run also
// fails on a wrong answer, not only on a bad access.  Without an argument a small built-in batch runs.  Exit status 0 and "ok" =
// clean.
#include "emu_align.cpp"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <tuple>

namespace {

int code_of(char c) { return c == 'C' ? 1 : c == 'T' ? 2 : c == 'G' ? 3 : 0; }

struct Pair { std::string q; int ref, centre, pile_row; };
struct Brute { int32_t stat[6]; std::vector<uint16_t> cols; };

const int BIG = 1 << 20;

Brute brute(const std::string& q, const std::string& r, int c, int span) {
    const int n = (int)q.size(), m = (int)r.size();
    Brute out;
    out.cols.assign((size_t)span, 7);
    auto in_band = [&](int i, int j) { return i >= 0 && i <= n && j >= 0 && j <= m && j - i >= c - 32 && j - i <= c + 31; };
    // the band's cells of every row: j = i + c - 32 .. i + c + 31
    std::vector<std::vector<int>> D((size_t)(n + 1), std::vector<int>(64, BIG));
    auto at = [&](int i, int j) { return in_band(i, j) ? D[(size_t)i][(size_t)(j - i - c + 32)] : BIG; };
    for (int i = 0; i <= n; ++i)
        for (int l = 0; l < 64; ++l) {
            const int j = i + c - 32 + l;
            if (!in_band(i, j)) continue;
            int d = BIG;
            if (i == 0 || j == 0) d = 0;
            else {
                d = std::min(d, at(i - 1, j - 1) + (code_of(q[(size_t)(i - 1)]) != code_of(r[(size_t)(j - 1)]) ? 1 : 0));
                d = std::min(d, at(i - 1, j) + 1);
                d = std::min(d, at(i, j - 1) + 1);
                d = std::min(d, BIG);
            }
            D[(size_t)i][(size_t)l] = d;
        }
    std::tuple<int, int, int> best(BIG, 0, 0);
    for (int i = 0; i <= n; ++i)
        for (int l = 0; l < 64; ++l) {
            const int j = i + c - 32 + l;
            if (!in_band(i, j) || (i != n && j != m) || at(i, j) >= BIG) continue;
            best = std::min(best, std::make_tuple(at(i, j), -i, -j));
        }
    if (std::get<0>(best) >= BIG) {
        const int32_t none[6] = {0, 0, 0, 0, 0, 1};
        std::copy(none, none + 6, out.stat);
        return out;
    }
    int i = -std::get<1>(best), j = -std::get<2>(best), flags = 0;
    const int q_end = i, r_end = j;
    std::vector<int> ins;
    while (i > 0 && j > 0) {
        const int l = j - i - c + 32;
        if (l == 0 || l == 63) flags |= 2;
        const int s = code_of(q[(size_t)(i - 1)]) != code_of(r[(size_t)(j - 1)]) ? 1 : 0;
        if (at(i - 1, j - 1) < BIG && at(i, j) == at(i - 1, j - 1) + s) {
            out.cols[(size_t)(j - 1)] = (uint16_t)code_of(q[(size_t)(i - 1)]);
        } else if (at(i - 1, j) < BIG && at(i, j) == at(i - 1, j) + 1) {
            ins.insert(ins.begin(), code_of(q[(size_t)(i - 1)]));
            --i;
            continue;
        } else {
            out.cols[(size_t)(j - 1)] = 4;
        }
        if (!ins.empty() && j < r_end)
            out.cols[(size_t)j] = (uint16_t)(out.cols[(size_t)j] | std::min((int)ins.size(), 3) << 3 | ins[0] << 5 | (ins.size() >= 2 ? ins[1] << 7 : 0));
        ins.clear();
        if (out.cols[(size_t)(j - 1)] != 4) --i;
        --j;
    }
    const int32_t st[6] = {std::get<0>(best), i, q_end, j, r_end, flags};
    std::copy(st, st + 6, out.stat);
    return out;
}

void pack(const std::vector<std::string>& ws, int span, std::vector<uint32_t>& codes, std::vector<int32_t>& length) {
    const int cdw = (span + 15) / 16;
    codes.assign(ws.size() * (size_t)cdw, 0);
    length.clear();
    for (size_t r = 0; r < ws.size(); ++r) {
        for (size_t p = 0; p < ws[r].size(); ++p) codes[r * (size_t)cdw + (p >> 4)] |= (uint32_t)code_of(ws[r][p]) << (2 * (p & 15));
        length.push_back((int32_t)ws[r].size());
    }
}

// mode: 0 = everything, 1 = no cols, 2 = no pile, 3 = neither
int run_case(const std::vector<std::string>& refs, const std::vector<Pair>& pairs, int span, int n_pile, int mode, long& checked) {
    std::vector<std::string> qs;
    std::vector<int32_t> ref, centre, prow;
    for (const Pair& p : pairs) { qs.push_back(p.q); ref.push_back(p.ref); centre.push_back(p.centre); prow.push_back(p.pile_row); }
    std::vector<uint32_t> codes, rcodes;
    std::vector<int32_t> length, rlength;
    pack(qs, span, codes, length);
    pack(refs, span, rcodes, rlength);
    const int64_t n = (int64_t)pairs.size();
    const bool want_cols = !(mode & 1), want_pile = !(mode & 2) && n_pile > 0;
    std::vector<int32_t> stat((size_t)(6 * n)), pile(want_pile ? (size_t)n_pile * (size_t)span * 13 : 0, 77);
    std::vector<uint16_t> cols(want_cols ? (size_t)(n * span) : 0);
    const int rc = emu_window_align(codes.data(), (int64_t)codes.size(), length.data(), n, rcodes.data(), (int64_t)rcodes.size(), rlength.data(), (int32_t)refs.size(),
                                    ref.data(), centre.data(), span, stat.data(), 6 * n, want_cols ? cols.data() : nullptr, (int64_t)cols.size(),
                                    want_pile ? prow.data() : nullptr, want_pile ? pile.data() : nullptr, want_pile ? n_pile : 0, (int64_t)pile.size());
    if (rc != TPS_OK) { printf("align: rc %d (%s)\n", rc, emu_align_last_error()); return 1; }
    std::vector<int32_t> want_p(pile.size(), 0);
    for (int64_t i = 0; i < n; ++i) {
        Brute b;
        if (ref[(size_t)i] >= 0) b = brute(qs[(size_t)i], refs[(size_t)ref[(size_t)i]], centre[(size_t)i], span);
        else {
            const int32_t none[6] = {0, 0, 0, 0, 0, 1};
            std::copy(none, none + 6, b.stat);
            b.cols.assign((size_t)span, 7);
        }
        if (!std::equal(b.stat, b.stat + 6, stat.begin() + 6 * i)) {
            printf("span %d pair %lld: stat %d %d %d %d %d %d, want %d %d %d %d %d %d\n", span, (long long)i, stat[6 * i], stat[6 * i + 1], stat[6 * i + 2],
                   stat[6 * i + 3], stat[6 * i + 4], stat[6 * i + 5], b.stat[0], b.stat[1], b.stat[2], b.stat[3], b.stat[4], b.stat[5]);
            return 1;
        }
        if (want_cols && !std::equal(b.cols.begin(), b.cols.end(), cols.begin() + i * span)) { printf("span %d pair %lld: the columns differ\n", span, (long long)i); return 1; }
        if (want_pile && prow[(size_t)i] >= 0 && b.stat[5] == 0)
            for (int j = b.stat[3]; j < b.stat[4]; ++j) {
                const int v = b.cols[(size_t)j];
                int32_t* col = want_p.data() + ((size_t)prow[(size_t)i] * (size_t)span + (size_t)j) * 13;
                ++col[v & 7];
                if ((v >> 3) & 3) ++col[5 + ((v >> 5) & 3)];
                if (((v >> 3) & 3) >= 2) ++col[9 + ((v >> 7) & 3)];
            }
        ++checked;
    }
    if (want_p != pile) { printf("span %d: the pile differs\n", span); return 1; }
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
            int span, n_pile;
            long n_ref, n;
            if (!(hd >> tag >> span >> n_ref >> n >> n_pile) || tag != "acase") { printf("bad case line: %s\n", line.c_str()); return 1; }
            std::vector<std::string> refs;
            std::vector<Pair> pairs;
            for (long i = 0; i < n_ref; ++i) {
                if (!std::getline(in, line)) { printf("the file ends inside a case\n"); return 1; }
                refs.push_back(line == "-" ? "" : line);
            }
            for (long i = 0; i < n; ++i) {
                if (!std::getline(in, line)) { printf("the file ends inside a case\n"); return 1; }
                std::istringstream rl(line);
                Pair p;
                if (!(rl >> p.ref >> p.centre >> p.pile_row >> p.q)) { printf("bad pair line\n"); return 1; }
                if (p.q == "-") p.q.clear();
                pairs.push_back(p);
            }
            if (run_case(refs, pairs, span, n_pile, n_cases & 3, checked)) return 1;
            ++n_cases;
        }
    } else {
        uint32_t x = 2424;
        auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
        for (int span : {1, 17, 333, 4096}) {
            std::string base;
            for (int i = 0; i < span + 100; ++i) base.push_back("ACGT"[rnd() & 3]);
            std::vector<std::string> refs{base.substr(0, (size_t)span), base.substr(0, (size_t)(span / 2)), ""};
            std::vector<Pair> pairs;
            for (int t = 0; t < 12; ++t) {
                std::string q;
                for (int i = 0; i < span + 100 && (int)q.size() < span; ++i) {
                    if (rnd() % 30u == 0) continue;
                    q.push_back(rnd() % 30u == 0 ? "ACGT"[rnd() & 3] : base[(size_t)i]);
                    if (rnd() % 30u == 0 && (int)q.size() < span) q.push_back("ACGT"[rnd() & 3]);
                }
                if (t == 3) q = q.substr(0, q.size() / 3);
                pairs.push_back(Pair{q, t == 5 ? -1 : t % 3, t == 7 ? 40 : t == 8 ? -4096 : (int)(rnd() % 9u) - 4, t % 4 == 3 ? -1 : t % 2});
            }
            for (int mode = 0; mode < 4; ++mode)
                if (run_case(refs, pairs, span, 2, mode, checked)) return 1;
            ++n_cases;
        }
    }
    // the refusals, and an empty call
    uint32_t co[14] = {0}, rco[21] = {0};
    int32_t st[12], pl[2600];
    uint16_t cl[200];
    auto call = [&](int64_t n, int n_ref, int span, int n_pile, int l0, int rl1, int r0, int c0, int p0, int64_t cl_len, int64_t pl_len) {
        const int32_t len[2] = {l0, 5}, rlen[3] = {100, rl1, 50}, ref[2] = {r0, -7}, ce[2] = {c0, -4096}, pr[2] = {p0, -1};
        return emu_window_align(co, 14, len, n, rco, 21, rlen, n_ref, ref, ce, span, st, 12, cl, cl_len, pr, pl, n_pile, pl_len);
    };
    // (row 0 meets an empty reference: its cells with j = 0 are end cells of D 0, the one with the largest i is (32, 0))
    if (call(2, 3, 100, 2, 100, 0, 1, 0, 1, 200, 2600) != TPS_OK || st[0] != 0 || st[1] != 32 || st[2] != 32 || st[4] != 0 || st[5] != 0 || st[11] != 1 || cl[0] != 7 || cl[199] != 7 || pl[0] != 0 || pl[2599] != 0) return 1;
    if (call(262145, 3, 100, 2, 100, 0, 1, 0, 1, 200, 2600) != TPS_E_CAPACITY || call(2, 0, 100, 2, 100, 0, 1, 0, 1, 200, 2600) != TPS_E_CAPACITY) return 1;
    if (call(2, 3, 0, 2, 100, 0, 1, 0, 1, 200, 2600) != TPS_E_CAPACITY || call(2, 3, 4097, 2, 100, 0, 1, 0, 1, 200, 2600) != TPS_E_CAPACITY) return 1;
    if (call(2, 3, 100, 4, 100, 0, 1, 0, 1, 200, 2600) != TPS_E_CAPACITY || call(2, 3, 100, -1, 100, 0, 1, 0, 1, 200, 2600) != TPS_E_CAPACITY) return 1;
    if (call(2, 3, 100, 2, 101, 0, 1, 0, 1, 200, 2600) != TPS_E_ARG || call(2, 3, 100, 2, 100, 101, 1, 0, 1, 200, 2600) != TPS_E_ARG) return 1;
    if (call(2, 3, 100, 2, 100, 0, 3, 0, 1, 200, 2600) != TPS_E_ARG || call(2, 3, 100, 2, 100, 0, 1, 4097, 1, 200, 2600) != TPS_E_ARG) return 1;
    if (call(2, 3, 100, 2, 100, 0, 1, 0, 2, 200, 2600) != TPS_E_ARG || call(2, 3, 100, 2, 100, 0, 1, 0, 1, 199, 2600) != TPS_E_ARG) return 1;
    if (call(2, 3, 100, 2, 100, 0, 1, 0, 1, 200, 2599) != TPS_E_ARG || call(2, 3, 100, 0, 100, 0, 1, 0, 1, 200, 0) != TPS_E_ARG) return 1;
    pl[5] = 9;
    if (emu_window_align(nullptr, 0, nullptr, 0, nullptr, 21, nullptr, 3, nullptr, nullptr, 100, nullptr, 0, nullptr, 0, nullptr, pl, 2, 2600) != TPS_E_ARG) return 1;
    const int32_t none[1] = {0};
    if (emu_window_align(nullptr, 0, nullptr, 0, nullptr, 21, nullptr, 3, nullptr, nullptr, 100, nullptr, 0, nullptr, 0, none, pl, 2, 2600) != TPS_OK || pl[5] != 0) return 1;
    printf("ok %d cases, %ld pairs\n", n_cases, checked);
    return 0;
}
