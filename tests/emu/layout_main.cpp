// TEST INFRASTRUCTURE ONLY -- the layout accumulator of the read-analysis calls (tps::Layout, topsicle_amd/csrc/tps_layout.h) against
// the offsets the library computed by hand before it had one.  A program of its own for -fsanitize=address,undefined; the add()
// sequences are the ones topsicle_hip.hip makes, the expected offsets are written out as the formulas that stood at each call.
#include <cstdio>
#include <vector>

#include "../../include/topsicle_hip.h"
#include "../../topsicle_amd/csrc/tps_layout.h"

struct Piece { size_t off, bytes, align; };

static int g_bad = 0;
#define EXPECT(cond)                                                                             \
    do {                                                                                         \
        if (!(cond)) { printf("line %d, n %lld, n_pat %d: %s\n", __LINE__, (long long)g_n, g_n_pat, #cond); ++g_bad; } \
    } while (0)
static long long g_n = 0;
static int g_n_pat = 0;

// every piece aligned as asked, no two overlapping (they were handed out in order), the total the sum the parent passed to ensure
static void check(const std::vector<Piece>& pieces, const tps::Layout& l, size_t want_total) {
    size_t end = 0;
    for (const Piece& p : pieces) {
        EXPECT(p.off % p.align == 0);
        EXPECT(p.off >= end);
        end = p.off + p.bytes;
    }
    EXPECT(l.total == end);
    EXPECT(l.total == want_total);
}

static void one(int64_t n, int n_pat) {
    g_n = n;
    g_n_pat = n_pat;
    const size_t N = (size_t)n;
    {   // tails / begin / end: variant census, end sketch, end window
        tps::Layout l;
        const tps::RegionAt r = tps::region_layout(l, n);
        const size_t off_begin = ((N + 15) & ~(size_t)15), off_end = off_begin + N * 4;
        EXPECT(r.tails == 0 && r.begin == off_begin && r.end == off_end);
        check({{r.tails, N, 16}, {r.begin, N * 4, 16}, {r.end, N * 4, 4}}, l, off_end + N * 4);
    }
    {   // adapter find: Peq, the lengths, then the region
        tps::Layout l;
        const size_t peq_bytes = (size_t)n_pat * 32, len_bytes = (size_t)n_pat * 4;
        const size_t peq = l.add(peq_bytes), len = l.add(len_bytes);
        const tps::RegionAt r = tps::region_layout(l, n);
        const size_t off_len = peq_bytes, off_tails = (off_len + len_bytes + 15) & ~(size_t)15, off_begin = (off_tails + N + 15) & ~(size_t)15,
                     off_end = off_begin + N * 4;
        EXPECT(peq == 0 && len == off_len && r.tails == off_tails && r.begin == off_begin && r.end == off_end);
        check({{peq, peq_bytes, 8}, {len, len_bytes, 4}, {r.tails, N, 16}, {r.begin, N * 4, 16}, {r.end, N * 4, 4}}, l, off_end + N * 4);
    }
    {   // tract map: tracts, found, totals
        const int max_tracts = 3;
        tps::Layout l;
        const size_t tr_bytes = N * 2 * max_tracts * sizeof(tps_tract), fo_bytes = N * 2 * 4, to_bytes = N * 4 * 4;
        const size_t tr = l.add(tr_bytes), fo = l.add(fo_bytes), to = l.add(to_bytes);
        EXPECT(tr == 0 && fo == tr_bytes && to == tr_bytes + fo_bytes);
        check({{tr, tr_bytes, 4}, {fo, fo_bytes, 4}, {to, to_bytes, 4}}, l, tr_bytes + fo_bytes + to_bytes);
    }
    {   // sketch links: degree, links, matches
        const int max_links = 5;
        tps::Layout l;
        const size_t dg_bytes = N * 4, ln_bytes = N * max_links * 4;
        const size_t dg = l.add(dg_bytes), ln = l.add(ln_bytes), ma = l.add(ln_bytes);
        EXPECT(dg == 0 && ln == dg_bytes && ma == dg_bytes + ln_bytes);
        check({{dg, dg_bytes, 4}, {ln, ln_bytes, 4}, {ma, ln_bytes, 4}}, l, dg_bytes + 2 * ln_bytes);
    }
    const int span = 100, cdw = (span + 15) / 16, kdw = (span + 31) / 32;
    const size_t co_bytes = N * cdw * 4, kp_bytes = N * kdw * 4, n_bytes = N * 4;
    {   // end sketch: sketch, kept; end window: codes, keep
        const int buckets = 128;
        tps::Layout s, w;
        const size_t sk_bytes = N * buckets * 4, kept_bytes = N * 4;
        const size_t sk = s.add(sk_bytes), kp = s.add(kept_bytes);
        EXPECT(sk == 0 && kp == sk_bytes);
        check({{sk, sk_bytes, 4}, {kp, kept_bytes, 4}}, s, sk_bytes + kept_bytes);
        const size_t co = w.add(co_bytes), ke = w.add(kp_bytes);
        EXPECT(co == 0 && ke == co_bytes);
        check({{co, co_bytes, 4}, {ke, kp_bytes, 4}}, w, co_bytes + kp_bytes);
    }
    {   // window offsets: codes, keep, length, ref in; offset, votes, second out
        tps::Layout in, out;
        const size_t co = in.add(co_bytes), ke = in.add(kp_bytes), le = in.add(n_bytes), re = in.add(n_bytes);
        EXPECT(co == 0 && ke == co_bytes && le == co_bytes + kp_bytes && re == co_bytes + kp_bytes + n_bytes);
        check({{co, co_bytes, 4}, {ke, kp_bytes, 4}, {le, n_bytes, 4}, {re, n_bytes, 4}}, in, co_bytes + kp_bytes + 2 * n_bytes);
        const size_t of = out.add(n_bytes), vo = out.add(n_bytes), se = out.add(n_bytes);
        EXPECT(of == 0 && vo == n_bytes && se == 2 * n_bytes);
        check({{of, n_bytes, 4}, {vo, n_bytes, 4}, {se, n_bytes, 4}}, out, 3 * n_bytes);
    }
    for (const size_t key_bytes : {(size_t)0, (size_t)20}) {   // window place: codes, keep, length in; dir, keys, ent of the index (keys and ent may be empty)
        tps::Layout in, idx;
        const size_t dir_bytes = 16 * 4 + 4, ent_bytes = key_bytes ? 36 : 0;
        const size_t co = in.add(co_bytes), ke = in.add(kp_bytes), le = in.add(n_bytes);
        EXPECT(co == 0 && ke == co_bytes && le == co_bytes + kp_bytes);
        check({{co, co_bytes, 4}, {ke, kp_bytes, 4}, {le, n_bytes, 4}}, in, co_bytes + kp_bytes + n_bytes);
        const size_t di = idx.add(dir_bytes), ky = idx.add(key_bytes), en = idx.add(ent_bytes);
        EXPECT(di == 0 && ky == dir_bytes && en == dir_bytes + key_bytes);
        check({{di, dir_bytes, 4}, {ky, key_bytes, 4}, {en, ent_bytes, 4}}, idx, dir_bytes + key_bytes + ent_bytes);
    }
}

int main() {
    int cases = 0;
    for (const int64_t n : {0, 1, 15, 16, 17, 4097})
        for (const int n_pat : {1, 63, 64}) { one(n, n_pat); ++cases; }
    if (g_bad) { printf("%d layout checks failed\n", g_bad); return 1; }
    printf("ok %d layouts\n", cases);
    return 0;
}
