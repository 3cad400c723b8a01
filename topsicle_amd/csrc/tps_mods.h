// tps_mods.h -- the base-modification tags of a BAM record (tps_bam_mods_spans, include/topsicle_io.h): the walk over the aux block
// (SAMv1 4.2.4: A c C s S i I f Z H B), the MM:Z grammar of SAMtags, ([ACGTUN][-+]([a-z]+|[0-9]+)[.?]?(,[0-9]+)*;)*, and the ML:B:C
// bytes that go with one group.  Plain C++ on a byte range, nothing else of the reader: tps_io.cpp includes it, and so does the
// stand-alone program the sanitizers run (tests/emu/mods_main.cpp).
//
// Out of scope, each answered with MODS_NOGROUP: groups on base N (or any base but C), the reverse strand (C-m: duplex reads), codes
// given as ChEBI numbers only.  The first group on C+ whose code list holds the code asked for is taken.  Nothing is reversed for a
// reverse-strand record: MM counts along the read as sequenced.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

namespace tps {

enum { MODS_OK = 0, MODS_NONE = 1, MODS_NOGROUP = 2, MODS_MALFORMED = 3, MODS_CLIPPED = 4 };

// bytes of a fixed-size aux value (0: none of them)
inline int mods_fixed_size(uint8_t type) {
    switch (type) {
        case 'A': case 'c': case 'C': return 1;
        case 's': case 'S': return 2;
        case 'i': case 'I': case 'f': return 4;
        default: return 0;
    }
}

// One record: aux[0 .. aux_len) is its aux block, l_seq its bases.  Returns the status; MODS_OK appends the group's skip counts to
// `delta` and its ML bytes to `prob` and sets *mode (1: '?', skipped bases unknown; 0: '.' or no flag, skipped bases unmodified).
// Precedence: a tag that runs past the block, MODS_MALFORMED; no MM:Z or no ML:B, MODS_NONE; an MM that does not follow the grammar or
// holds a count over 2^32 - 1, an ML:B that is not of bytes, an MN that is no integer, MODS_MALFORMED; no group to take, MODS_NOGROUP;
// ML shorter than all groups need, MODS_MALFORMED; MN that differs from l_seq, MODS_CLIPPED.
inline int mods_record(const uint8_t* aux, int64_t aux_len, int64_t l_seq, char code, uint8_t* mode, std::vector<uint32_t>& delta, std::vector<uint8_t>& prob) {
    const uint8_t *mm = nullptr, *ml = nullptr;
    int64_t mm_len = 0, ml_len = 0, mn = -1;
    bool have_mn = false, bad = false;
    for (int64_t p = 0; p < aux_len;) {
        if (p + 3 > aux_len) return MODS_MALFORMED;
        const uint8_t t0 = aux[p], t1 = aux[p + 1], type = aux[p + 2];
        p += 3;
        int64_t n = mods_fixed_size(type);
        if (type == 'Z' || type == 'H') {
            const void* z = memchr(aux + p, 0, (size_t)(aux_len - p));
            if (!z) return MODS_MALFORMED;
            n = (const uint8_t*)z - (aux + p) + 1;
        } else if (type == 'B') {
            if (p + 5 > aux_len) return MODS_MALFORMED;
            const int sz = aux[p] == 'A' ? 0 : mods_fixed_size(aux[p]);
            if (!sz) return MODS_MALFORMED;
            uint32_t count;
            memcpy(&count, aux + p + 1, 4);
            n = 5 + (int64_t)sz * count;
        } else if (n == 0) {
            return MODS_MALFORMED;
        }
        if (n > aux_len - p) return MODS_MALFORMED;
        if (t0 == 'M' && t1 == 'M' && type == 'Z' && !mm) {
            mm = aux + p;
            mm_len = n - 1;
        } else if (t0 == 'M' && t1 == 'L' && type == 'B' && !ml) {
            if (aux[p] != 'C') bad = true;
            ml = aux + p + 5;
            ml_len = n - 5;
        } else if (t0 == 'M' && t1 == 'N' && !have_mn) {
            have_mn = true;
            if (type == 'c') mn = (int8_t)aux[p];
            else if (type == 'C') mn = aux[p];
            else if (type == 's') { int16_t v; memcpy(&v, aux + p, 2); mn = v; }
            else if (type == 'S') { uint16_t v; memcpy(&v, aux + p, 2); mn = v; }
            else if (type == 'i') { int32_t v; memcpy(&v, aux + p, 4); mn = v; }
            else if (type == 'I') { uint32_t v; memcpy(&v, aux + p, 4); mn = v; }
            else bad = true;
        }
        p += n;
    }
    if (bad) return MODS_MALFORMED;
    if (!mm || !ml) return MODS_NONE;
    // the groups: where each one's ML bytes start, and the first one to take
    int64_t at = 0, take_at = -1, take_codes = 0, take_which = 0;
    uint8_t take_flag = 0;
    std::vector<uint32_t> counts;
    for (int64_t p = 0; p < mm_len;) {
        const uint8_t base = mm[p];
        if (!memchr("ACGTUN", base, 6) || p + 1 >= mm_len || (mm[p + 1] != '+' && mm[p + 1] != '-')) return MODS_MALFORMED;
        const bool plus = mm[p + 1] == '+';
        int64_t q = p + 2, which = -1;
        while (q < mm_len && mm[q] >= 'a' && mm[q] <= 'z') {
            if (which < 0 && mm[q] == (uint8_t)code) which = q - (p + 2);
            ++q;
        }
        int64_t n_codes = q - (p + 2);
        if (n_codes == 0) {                            // a ChEBI number
            while (q < mm_len && mm[q] >= '0' && mm[q] <= '9') ++q;
            if (q == p + 2) return MODS_MALFORMED;
            n_codes = 1;
            which = -1;
        }
        uint8_t flag = 0;
        if (q < mm_len && (mm[q] == '.' || mm[q] == '?')) flag = mm[q++];
        const bool take = take_at < 0 && base == 'C' && plus && which >= 0;
        int64_t n_counts = 0;
        while (q < mm_len && mm[q] == ',') {
            int64_t d = q + 1;
            uint64_t v = 0;
            while (d < mm_len && mm[d] >= '0' && mm[d] <= '9') {
                if (v <= 0xFFFFFFFFull) v = v * 10 + (uint64_t)(mm[d] - '0');     // (past 2^32 it only has to stay there)
                ++d;
            }
            if (d == q + 1 || v > 0xFFFFFFFFull) return MODS_MALFORMED;
            if (take) counts.push_back((uint32_t)v);
            ++n_counts;
            q = d;
        }
        if (q >= mm_len || mm[q] != ';') return MODS_MALFORMED;
        if (take) { take_at = at; take_codes = n_codes; take_which = which; take_flag = flag; }
        at += n_codes * n_counts;
        p = q + 1;
    }
    if (take_at < 0) return MODS_NOGROUP;
    if (at > ml_len) return MODS_MALFORMED;
    if (have_mn && mn != l_seq) return MODS_CLIPPED;
    *mode = take_flag == '?' ? 1 : 0;
    delta.insert(delta.end(), counts.begin(), counts.end());
    for (size_t i = 0; i < counts.size(); ++i) prob.push_back(ml[take_at + (int64_t)i * take_codes + take_which]);
    return MODS_OK;
}

// tps_bam_mods_spans without the error text: -1 and *why on a bad span, -2 when mods_cap is too small, else the entries.  Nothing is
// written unless everything fits.
inline int64_t mods_spans(const char* text, int64_t text_len, const int64_t* spans, const int32_t* lens, const int64_t* idx, int64_t n_idx, char code,
                          int32_t* status, uint8_t* mode, int64_t* mod_off, uint32_t* delta, uint8_t* prob, int64_t mods_cap, const char** why) {
    if (!text || !spans || !lens || (n_idx > 0 && (!idx || !status || !mode)) || !mod_off || n_idx < 0 || mods_cap < 0) { *why = "null argument"; return -1; }
    if (code < 'a' || code > 'z') { *why = "the modification code must be a lower-case letter"; return -1; }
    std::vector<uint32_t> d;
    std::vector<uint8_t> p, md((size_t)n_idx, 0);
    std::vector<int32_t> st((size_t)n_idx, 0);
    std::vector<int64_t> off((size_t)n_idx + 1, 0);
    for (int64_t j = 0; j < n_idx; ++j) {
        const int64_t i = idx[j];
        if (i < 0) { *why = "negative record index"; return -1; }
        const int64_t h0 = spans[4 * i], q0 = spans[4 * i + 3], L = lens[i];
        // the record starts 36 bytes in front of its name: block_size, then the 32 fixed bytes; its aux block lies behind the qualities
        if (h0 < 36 || h0 > text_len || q0 < h0 || L < 0 || q0 > text_len - L) { *why = "record span outside the text"; return -1; }
        int32_t block_size, l_seq;
        memcpy(&block_size, text + h0 - 36, 4);
        memcpy(&l_seq, text + h0 - 16, 4);
        const int64_t rec_end = h0 - 32 + (int64_t)block_size;
        if (block_size < 32 || rec_end > text_len || q0 + L > rec_end) { *why = "record span outside the text"; return -1; }
        st[(size_t)j] = mods_record((const uint8_t*)text + q0 + L, rec_end - (q0 + L), l_seq, code, &md[(size_t)j], d, p);
        off[(size_t)j + 1] = (int64_t)d.size();
    }
    if ((int64_t)d.size() > mods_cap) return -2;
    if (n_idx > 0) {
        memcpy(status, st.data(), st.size() * 4);
        memcpy(mode, md.data(), md.size());
    }
    memcpy(mod_off, off.data(), off.size() * 8);
    if (!d.empty()) {
        if (!delta || !prob) { *why = "null argument"; return -1; }
        memcpy(delta, d.data(), d.size() * 4);
        memcpy(prob, p.data(), p.size());
    }
    return (int64_t)d.size();
}

}  // namespace tps
