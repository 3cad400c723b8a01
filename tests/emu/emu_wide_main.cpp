// TEST INFRASTRUCTURE ONLY -- the wide-table scan emulation (emu_wide.cpp) as a stand-alone program for the sanitizers:
//   g++ -fsanitize=address,undefined emu_wide_main.cpp && ./a.out ROWS_FILE
// ROWS_FILE holds the rows of tests/wide_path_rows.py with their reads (wide_path_rows.dump_rows writes it, the format is there).
// Every row is scanned at the four alignments of the batch inside its buffer, with every output buffer exactly as large as the
// layout says and the LDS slice exactly as large as the plan says, so an access past either is seen; the return code is compared
// with the row's, and a digest of the outputs with the one the file carries (taken from the scan that was compared with
// oracle/oracle.c), so that the run also fails on a wrong answer.  Exit status 0 and "ok: N rows" = clean.
#include "emu_wide.cpp"

#include <cstdio>

namespace {

template <class T>
bool get(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

// what wide_path_rows.digest computes: the decision and change point of every read, S_w and raw bytes of the reads that passed
uint64_t digest(const tps_params& prm, int P, int64_t n, const tps_read_result* res, const int32_t* cs, const int32_t* ce,
                const int64_t* wo, const int32_t* sums, const uint8_t* raw) {
    int64_t d = 0;
    for (int64_t i = 0; i < n; ++i) {
        const tps_read_result& r = res[i];
        d += (int64_t)r.pass + 3 * (int64_t)r.tail + 5 * (int64_t)r.n_win + 7 * (int64_t)r.bkp + 11 * (int64_t)r.best_start + 13 * (int64_t)r.best_end;
        if (prm.flags & TPS_F_STEP1)
            for (int p = 0; p < P; ++p) d += 23 * (int64_t)cs[i * P + p] + 29 * (int64_t)ce[i * P + p];
        if (!r.pass || !(prm.flags & TPS_F_WINDOWS)) continue;
        for (int64_t w = wo[i]; w < wo[i + 1]; ++w) {
            d += 17 * (int64_t)sums[w];
            if (prm.flags & TPS_F_STORE_RAW)
                for (int p = 0; p < P; ++p) d += 19 * (int64_t)raw[w * P + p];
        }
    }
    return (uint64_t)d;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s ROWS_FILE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[3];
    int nrow = 0;
    while (fread(hdr, 4, 3, f) == 3) {
        const int P = hdr[0], k = hdr[1], refuse = hdr[2];
        std::vector<char> pats((size_t)P * (size_t)k);
        tps_params prm;
        int64_t n = 0;
        uint64_t want = 0;
        if (!get(f, pats.data(), pats.size()) || !get(f, &prm, 1) || !get(f, &want, 1) || !get(f, &n, 1)) { fprintf(stderr, "row %d: short file\n", nrow); return 2; }
        std::vector<int64_t> off((size_t)n + 1);
        if (!get(f, off.data(), off.size())) { fprintf(stderr, "row %d: short file\n", nrow); return 2; }
        const size_t nb = (size_t)off[(size_t)n];
        // malloc'd, exactly sized: the sanitizer's red zones start at the first byte past each
        uint8_t* bases = (uint8_t*)malloc(nb ? nb : 1);
        uint8_t* tails = (uint8_t*)malloc(n ? (size_t)n : 1);
        if (!get(f, bases, nb) || !get(f, tails, (size_t)n)) { fprintf(stderr, "row %d: short file\n", nrow); return 2; }
        int64_t tot = 0;
        for (int64_t i = 0; i < n; ++i) tot += tps::window_count(off[(size_t)i + 1] - off[(size_t)i], prm.window, prm.slide, prm.trimfirst, prm.maxlen);
        tps_read_result* res = (tps_read_result*)malloc(sizeof(tps_read_result) * (size_t)(n ? n : 1));
        int32_t* cs = (int32_t*)malloc(4 * (size_t)(n * P ? n * P : 1));
        int32_t* ce = (int32_t*)malloc(4 * (size_t)(n * P ? n * P : 1));
        int64_t* wo = (int64_t*)malloc(8 * (size_t)(n + 1));
        int32_t* sums = (int32_t*)malloc(4 * (size_t)(tot ? tot : 1));
        uint8_t* raw = (uint8_t*)malloc((size_t)(tot * P ? tot * P : 1));
        for (int shift = 0; shift < 4; ++shift) {
            const int rc = emu_wide_scan(pats.data(), P, k, bases, off.data(), n, tails, &prm, shift, res, cs, ce, wo, sums, raw);
            if (rc != refuse) { printf("row %d shift %d: rc %d, expected %d (%s)\n", nrow, shift, rc, refuse, emu_wide_last_error()); return 1; }
            if (rc == TPS_OK) {
                const uint64_t got = digest(prm, P, n, res, cs, ce, wo, sums, raw);
                if (got != want) { printf("row %d shift %d: digest %llu, expected %llu\n", nrow, shift, (unsigned long long)got, (unsigned long long)want); return 1; }
            }
        }
        free(bases); free(tails); free(res); free(cs); free(ce); free(wo); free(sums); free(raw);
        ++nrow;
    }
    fclose(f);
    printf("ok: %d rows\n", nrow);
    return 0;
}
