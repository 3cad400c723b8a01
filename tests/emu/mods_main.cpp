// TEST INFRASTRUCTURE ONLY -- the aux walk of the native reader (tps_bam_mods_spans; topsicle_amd/csrc/tps_mods.h) as a stand-alone
// program for the sanitizers:
//   g++ -fsanitize=address,undefined mods_main.cpp && ./a.out TEXT SPANS
// TEXT holds BAM records behind one another as the reader's window of inflated text holds them (tests/test_methyl.py writes the
// records of its aux cases into it); SPANS is a text file: the modification code, then one line per record with name offset, name
// length, seq offset, qual offset and bases.  The text sits in a buffer of exactly its size, so a walk that leaves a record at the
// very end of the window is seen.  Prints one line per record -- status, mode, the entries as delta:prob -- then, for a capacity one
// too small, that -2 came back with nothing written, then "ok".
#include "../../topsicle_amd/csrc/tps_mods.h"

#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: mods_main TEXT SPANS\n"); return 2; }
    std::ifstream tf(argv[1], std::ios::binary);
    std::ifstream sf(argv[2]);
    if (!tf || !sf) { printf("cannot read the inputs\n"); return 2; }
    const std::string all((std::istreambuf_iterator<char>(tf)), std::istreambuf_iterator<char>());
    std::vector<char> text(all.begin(), all.end());             // exactly the window
    std::string code;
    sf >> code;
    std::vector<int64_t> spans, idx;
    std::vector<int32_t> lens;
    long long h0, hl, s0, q0, L;
    while (sf >> h0 >> hl >> s0 >> q0 >> L) {
        idx.push_back((int64_t)lens.size());
        spans.insert(spans.end(), {h0, hl, s0, q0});
        lens.push_back((int32_t)L);
    }
    const int64_t n = (int64_t)idx.size();
    std::vector<int32_t> status((size_t)n, -9);
    std::vector<uint8_t> mode((size_t)n, 9);
    std::vector<int64_t> off((size_t)n + 1, -9);
    const char* why = "";
    // first with no room at all: the count comes from a second call with exactly enough
    std::vector<uint32_t> none;
    int64_t got = tps::mods_spans(text.data(), (int64_t)text.size(), spans.data(), lens.data(), idx.data(), n, code[0], status.data(), mode.data(), off.data(),
                                  nullptr, nullptr, 0, &why);
    if (got == -1) { printf("error: %s\n", why); return 1; }
    int64_t total = 0;
    if (got == -2) {
        if (status[0] != -9 || off[0] != -9) { printf("-2 wrote something\n"); return 1; }
        for (int64_t cap = 1; got == -2; cap *= 2) {
            std::vector<uint32_t> d((size_t)cap);
            std::vector<uint8_t> p((size_t)cap);
            got = tps::mods_spans(text.data(), (int64_t)text.size(), spans.data(), lens.data(), idx.data(), n, code[0], status.data(), mode.data(), off.data(), d.data(),
                                  p.data(), cap, &why);
        }
        total = got;
    }
    std::vector<uint32_t> delta((size_t)total);                 // exactly the entries
    std::vector<uint8_t> prob((size_t)total);
    if (total > 0) {
        std::vector<uint32_t> d1((size_t)total - 1);
        std::vector<uint8_t> p1((size_t)total - 1);
        std::vector<int32_t> st2((size_t)n, -9);
        if (tps::mods_spans(text.data(), (int64_t)text.size(), spans.data(), lens.data(), idx.data(), n, code[0], st2.data(), mode.data(), off.data(), d1.data(), p1.data(),
                            total - 1, &why) != -2 || st2[0] != -9) {
            printf("a capacity one too small was not refused\n");
            return 1;
        }
        printf("cap %lld: -2, nothing written\n", (long long)(total - 1));
    }
    got = tps::mods_spans(text.data(), (int64_t)text.size(), spans.data(), lens.data(), idx.data(), n, code[0], status.data(), mode.data(), off.data(), delta.data(),
                          prob.data(), total, &why);
    if (got != total) { printf("error: %lld entries, then %lld\n", (long long)total, (long long)got); return 1; }
    for (int64_t j = 0; j < n; ++j) {
        printf("%d %d", status[(size_t)j], mode[(size_t)j]);
        for (int64_t k = off[(size_t)j]; k < off[(size_t)j + 1]; ++k) printf(" %u:%u", delta[(size_t)k], prob[(size_t)k]);
        printf("\n");
    }
    printf("ok\n");
    return 0;
}
