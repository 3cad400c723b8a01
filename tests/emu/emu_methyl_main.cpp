// TEST INFRASTRUCTURE ONLY -- the base-modification emulation (emu_methyl.cpp) as a stand-alone program for the sanitizers:
//   g++ -fsanitize=address,undefined emu_methyl_main.cpp && ./a.out CASES
// CASES is a text file (tests/test_methyl.py writes the cases of tests/methyl_cases.py into it), one case after another:
//   mcase <w> <nb0> <nb1> <hi> <lo> <n_reads>
//   <tail> <begin> <end> <origin> <read> <n_entries> <delta> <prob> <delta> <prob> ...     n_reads lines; "-" is the empty read
// Every row and every bin is compared with the plain rule below (a string, a vector of the positions of its C's), so that the run
// also fails on a wrong answer, not only on a bad access.  The LDS slice is one wave's, poisoned, and the entries, the rows and the
// bins have exactly their sizes (emu_mod_profile).  Without an argument a small built-in batch runs.  Exit status 0 and "ok" = clean.
#include "emu_methyl.cpp"

#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

namespace {

struct Read { std::string seq; int tail, begin, end, origin; std::vector<uint32_t> delta; std::vector<uint8_t> prob; };

void brute(const Read& rd, int w, int nb0, int nb1, int hi, int lo, tps_mod_row& row, std::vector<tps_mod_bin>& bins) {
    const int nb = nb0 + nb1;
    bins.assign((size_t)nb, tps_mod_bin{0, 0, 0, 0, 0});
    row = tps_mod_row{0, 0, 0, 0, 0, 0, 0, 0};
    std::string s;
    for (char c : rd.seq) s.push_back((char)(c >= 'a' && c <= 'z' ? c - 32 : c));
    const long L = (long)s.size();
    const long b = rd.begin, e = std::min((long)rd.end, L);
    if (e <= b) return;
    std::vector<long> cs;
    for (long p = 0; p < L; ++p) if (s[(size_t)p] == 'C') cs.push_back(p);
    auto t_of = [&](long p) { return rd.tail ? L - 1 - p : p; };
    auto cpg = [&](long p) { return p + 1 < L && s[(size_t)p + 1] == 'G'; };
    auto bin_of = [&](long t) {
        const long d = t - rd.origin;
        return (size_t)((d >= 0 ? d / w : -((-d + w - 1) / w)) + nb0);      // the floor
    };
    for (long p : cs) if (t_of(p) >= b && t_of(p) < e && cpg(p)) ++bins[bin_of(t_of(p))].cpg;
    unsigned long long o = 0;
    for (size_t j = 0; j < rd.delta.size(); ++j) {
        o += (unsigned long long)rd.delta[j] + 1ull;
        if (o - 1 >= cs.size()) { ++row.beyond; continue; }
        const long p = cs[(size_t)(o - 1)];
        if (t_of(p) < b || t_of(p) >= e) continue;
        ++row.in_region;
        if (!cpg(p)) { ++row.off_context; continue; }
        tps_mod_bin& x = bins[bin_of(t_of(p))];
        ++x.called;
        x.sum += rd.prob[j];
        if (rd.prob[j] >= hi) ++x.high;
        if (rd.prob[j] <= lo) ++x.low;
    }
    if (row.beyond) bins.assign((size_t)nb, tps_mod_bin{0, 0, 0, 0, 0});
    row.c_total = (uint32_t)cs.size();
    row.entries = (uint32_t)rd.delta.size();
    for (const tps_mod_bin& x : bins) { row.cpg += x.cpg; row.called += x.called; }
    row.flags = row.beyond ? TPS_MOD_BAD : 0u;
}

int run_case(int w, int nb0, int nb1, int hi, int lo, const std::vector<Read>& reads, int shift, long& checked) {
    std::vector<uint8_t> bases, tails, prob;
    std::vector<int64_t> offsets{0}, mod_off{0};
    std::vector<int32_t> begin, end, origin;
    std::vector<uint32_t> delta;
    for (const Read& r : reads) {
        bases.insert(bases.end(), r.seq.begin(), r.seq.end());
        offsets.push_back((int64_t)bases.size());
        tails.push_back((uint8_t)r.tail); begin.push_back(r.begin); end.push_back(r.end); origin.push_back(r.origin);
        delta.insert(delta.end(), r.delta.begin(), r.delta.end());
        prob.insert(prob.end(), r.prob.begin(), r.prob.end());
        mod_off.push_back((int64_t)delta.size());
    }
    bases.push_back(0);
    const int64_t n = (int64_t)reads.size(), nb = nb0 + nb1;
    std::vector<tps_mod_row> rows((size_t)n);                    // exactly the rows and the bins
    std::vector<tps_mod_bin> bins((size_t)(n * nb));
    std::vector<uint32_t> d_exact(delta);                        // (data() of an empty vector may be null: the check wants pointers only with entries)
    const int rc = emu_mod_profile(bases.data(), offsets.data(), n, tails.data(), begin.data(), end.data(), origin.data(), n, mod_off.data(), d_exact.data(),
                                   prob.data(), (int64_t)delta.size(), w, nb0, nb1, hi, lo, shift, rows.data(), n, bins.data(), n * nb);
    if (rc != TPS_OK) { printf("rc %d (%s)\n", rc, emu_methyl_last_error()); return 1; }
    for (int64_t r = 0; r < n; ++r) {
        tps_mod_row want;
        std::vector<tps_mod_bin> wb;
        brute(reads[(size_t)r], w, nb0, nb1, hi, lo, want, wb);
        if (memcmp(&want, &rows[(size_t)r], sizeof want) != 0 || memcmp(wb.data(), &bins[(size_t)(r * nb)], (size_t)nb * sizeof(tps_mod_bin)) != 0) {
            const tps_mod_row& g = rows[(size_t)r];
            printf("read %lld: got row (%u %u %u %u %u %u %u %u), want (%u %u %u %u %u %u %u %u), or other bins\n", (long long)r, g.c_total, g.entries, g.beyond,
                   g.in_region, g.off_context, g.cpg, g.called, g.flags, want.c_total, want.entries, want.beyond, want.in_region, want.off_context, want.cpg,
                   want.called, want.flags);
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
            int w, nb0, nb1, hi, lo;
            long n;
            if (!(hd >> tag >> w >> nb0 >> nb1 >> hi >> lo >> n) || tag != "mcase") { printf("bad case line: %s\n", line.c_str()); return 1; }
            std::vector<Read> reads;
            for (long i = 0; i < n; ++i) {
                if (!std::getline(in, line)) { printf("the file ends inside a case\n"); return 1; }
                std::istringstream rl(line);
                Read r;
                long ne;
                if (!(rl >> r.tail >> r.begin >> r.end >> r.origin >> r.seq >> ne)) { printf("bad read line\n"); return 1; }
                if (r.seq == "-") r.seq.clear();
                for (long j = 0; j < ne; ++j) {
                    unsigned long long d;
                    int p;
                    if (!(rl >> d >> p)) { printf("bad entry\n"); return 1; }
                    r.delta.push_back((uint32_t)d);
                    r.prob.push_back((uint8_t)p);
                }
                reads.push_back(r);
            }
            if (run_case(w, nb0, nb1, hi, lo, reads, n_cases & 3, checked)) return 1;
            ++n_cases;
        }
    } else {
        uint32_t x = 4321;
        auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
        std::vector<Read> reads;
        const int lens[] = {0, 1, 15, 16, 17, 33, 63, 64, 65, 500, 1023, 1024, 1025, 4000, 9000, 20000};
        for (int L : lens) {
            Read r;
            for (int i = 0; i < L; ++i) {
                const unsigned u = rnd() % 40u;
                if (u < 3 && i + 1 < L) { r.seq += "CG"; ++i; }
                else if (u == 3) r.seq.push_back('N');
                else r.seq.push_back("ACGT"[rnd() & 3]);
            }
            if (L == 500) for (char& c : r.seq) c = (char)(c >= 'A' && c <= 'Z' ? c + 32 : c);
            r.tail = (int)(rnd() & 1);
            r.origin = (int)(rnd() % (unsigned)(L + 1));
            r.begin = std::max(0, r.origin - (int)(rnd() % 1001u));
            r.end = r.origin + (int)(rnd() % 4001u);
            long c = 0;
            for (char ch : r.seq) c += ch == 'C' || ch == 'c';
            for (long o = 0; o < c + 2; ++o)
                if (rnd() % 3u == 0) { r.delta.push_back((uint32_t)(rnd() % 3u)); r.prob.push_back((uint8_t)rnd()); }
            reads.push_back(r);
        }
        if (run_case(500, 2, 8, 205, 50, reads, 1, checked)) return 1;
        ++n_cases;
    }
    // the refusals, and an empty batch
    const uint8_t one_read[12] = {'C', 'G', 'C', 'T', 'A', 'A', 'C', 'G', 'C', 'T', 'A', 'C'};
    const int64_t off[2] = {0, 12}, mo[2] = {0, 2};
    const uint32_t dl[2] = {0, 1};
    const uint8_t pr[2] = {255, 0};
    tps_mod_row row[1];
    tps_mod_bin bin[4];
    auto call = [&](int tail, int b, int e, int o, int w, int nb0, int nb1, int hi, int lo, int64_t nr, int64_t nm, int64_t rl, int64_t bl) {
        const uint8_t t[1] = {(uint8_t)tail};
        const int32_t bb[1] = {b}, ee[1] = {e}, oo[1] = {o};
        return emu_mod_profile(one_read, off, 1, t, bb, ee, oo, nr, mo, dl, pr, nm, w, nb0, nb1, hi, lo, 0, row, rl, bin, bl);
    };
    if (call(0, 0, 12, 0, 16, 0, 1, 205, 50, 1, 2, 1, 1) != TPS_OK || row[0].c_total != 5 || row[0].called != 2 || bin[0].cpg != 2 || bin[0].high != 1 || bin[0].low != 1 ||
        bin[0].sum != 255)
        return 1;
    if (call(0, 0, 12, 0, 15, 0, 1, 205, 50, 1, 2, 1, 1) != TPS_E_CAPACITY || call(0, 0, 12, 0, 16, 0, 0, 205, 50, 1, 2, 1, 0) != TPS_E_CAPACITY) return 1;
    if (call(0, 0, 12, 0, 16, 0, 1, 50, 50, 1, 2, 1, 1) != TPS_E_ARG || call(2, 0, 12, 0, 16, 0, 1, 205, 50, 1, 2, 1, 1) != TPS_E_ARG) return 1;
    if (call(0, 0, 12, 0, 16, 0, 1, 205, 50, 2, 2, 1, 1) != TPS_E_ARG || call(0, 0, 12, 0, 16, 0, 1, 205, 50, 1, 3, 1, 1) != TPS_E_ARG) return 1;
    if (call(0, 0, 12, 0, 16, 0, 1, 205, 50, 1, 2, 2, 1) != TPS_E_ARG || call(0, 0, 12, 0, 16, 0, 1, 205, 50, 1, 2, 1, 2) != TPS_E_ARG) return 1;
    if (call(0, 0, 12, 4, 16, 0, 1, 205, 50, 1, 2, 1, 1) != TPS_E_ARG || call(0, 5, 4, 0, 16, 0, 1, 205, 50, 1, 2, 1, 1) != TPS_E_ARG) return 1;
    if (call(0, 0, 1 << 30, 0, 16, 0, 1, 205, 50, 1, 2, 1, 1) != TPS_OK) return 1;                  // (end far past the read: clamped before it is measured)
    if (emu_mod_profile(one_read, off, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 16, 0, 1, 205, 50, 0, nullptr, 0, nullptr, 0) != TPS_OK) return 1;
    printf("ok %d cases, %ld rows\n", n_cases, checked);
    return 0;
}
