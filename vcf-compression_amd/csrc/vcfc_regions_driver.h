// vcfc_regions_driver.h -- host side of region-list queries,
// shared by the C ABI (vcfc_api.cpp) and the CPU emulator harness
// (tests/simt_emu/emu_regions_api.cpp), so the same control flow is tested on
// both.
//
//   regions_build     region text -> the table blob (vcfc_device.h)
//   regions_validate  every count, offset and order the kernel relies on
//   regions_upload    validate, then copy the blob to the device
//   regions_step      the vcfc_dec::MatchStep that fills the flags from a
//                     table, for the three drivers that take one
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "vcfc_decode_driver.h"
#include "vcfc_device.h"

namespace vcfc_reg {

constexpr int ST_OK = 0, ST_E_NOSPACE = 4, ST_E_ARG = 5, ST_E_HIP = 6;   // = include/vcfc.h codes

// str_to_uint64 (reference src/utils.cpp:152-165: strtoul over the whole
// string; "" parses as 0)
inline bool str_to_u64(const char *s, uint64_t n, uint64_t *out) {
    if (n == 0) { *out = 0; return true; }
    uint64_t i = 0;
    while (i < n && (s[i] == ' ' || (s[i] >= '\t' && s[i] <= '\r'))) i++;
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; i++; }
    if (i >= n || s[i] < '0' || s[i] > '9') return false;
    uint64_t v = 0;
    bool ovf = false;
    for (; i < n && s[i] >= '0' && s[i] <= '9'; i++) {
        const uint64_t d = (uint64_t)(s[i] - '0');
        ovf = ovf || v > (UINT64_MAX - d) / 10;
        v = v * 10 + d;
    }
    if (i != n) return false;
    *out = ovf ? UINT64_MAX : (neg ? 0 - v : v);
    return true;
}

// parse_coordinate_string (reference src/main.cpp:3993-4026): 0, or 1 (no
// '-' after the ':'), 2 (start), 3 (end)
inline int parse_query(const char *q, uint64_t q_len, uint64_t *ref_len, int *has_range, uint64_t *start, uint64_t *end) {
    const char *colon = q_len ? static_cast<const char *>(memchr(q, ':', q_len)) : nullptr;
    if (!colon) {
        *ref_len = q_len; *has_range = 0; *start = *end = 0;
        return 0;
    }
    const uint64_t ci = (uint64_t)(colon - q);
    const char *dash = static_cast<const char *>(memchr(q + ci + 1, '-', q_len - ci - 1));
    if (!dash) return 1;
    const uint64_t di = (uint64_t)(dash - q);
    if (!str_to_u64(q + ci + 1, di - ci - 1, start)) return 2;
    if (!str_to_u64(q + di + 1, q_len - di - 1, end)) return 3;
    *ref_len = ci;
    *has_range = 1;
    return 0;
}

// a BED coordinate: 1..20 ASCII digits that fit 64 bits
inline bool bed_number(const char *s, uint64_t n, uint64_t *out) {
    if (n == 0 || n > 20) return false;
    uint64_t v = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (s[i] < '0' || s[i] > '9') return false;
        const uint64_t d = (uint64_t)(s[i] - '0');
        if (v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    *out = v;
    return true;
}

struct Region {
    std::string name;
    uint64_t start, end;   // inclusive; start > end: empty
};

// One line of a regions file (without its line end).  *skip: a blank or
// comment line.  false: it does not parse.
inline bool parse_line(const char *l, uint64_t n, Region *r, bool *skip) {
    *skip = n == 0 || l[0] == '#' || (n >= 5 && memcmp(l, "track", 5) == 0) || (n >= 7 && memcmp(l, "browser", 7) == 0);
    if (*skip) return true;
    const char *t1 = static_cast<const char *>(memchr(l, '\t', n));
    if (t1) {   // BED: name TAB start TAB end [TAB ...], 0-based and half-open
        const char *e = l + n;
        const char *t2 = static_cast<const char *>(memchr(t1 + 1, '\t', (size_t)(e - t1 - 1)));
        if (!t2) return false;
        const char *t3 = static_cast<const char *>(memchr(t2 + 1, '\t', (size_t)(e - t2 - 1)));
        if (!t3) t3 = e;
        uint64_t b0 = 0, b1 = 0;
        if (!bed_number(t1 + 1, (uint64_t)(t2 - t1 - 1), &b0) || !bed_number(t2 + 1, (uint64_t)(t3 - t2 - 1), &b1)) return false;
        r->name.assign(l, t1);
        if (b1 <= b0) { r->start = 1; r->end = 0; }
        else { r->start = b0 + 1; r->end = b1; }
        return true;
    }
    uint64_t ref_len = 0, start = 0, end = 0;
    int has_range = 0;
    if (parse_query(l, n, &ref_len, &has_range, &start, &end)) return false;
    r->name.assign(l, l + ref_len);
    r->start = has_range ? start : 0;
    r->end = has_range ? end : UINT64_MAX;
    return true;
}

// Region text -> regions.  false with *bad_line = the 1-based number of the
// first line that does not parse.
inline bool parse_text(const char *text, uint64_t len, std::vector<Region> &out, uint64_t *bad_line) {
    out.clear();
    uint64_t line = 0;
    for (uint64_t a = 0; a < len;) {
        const char *lf = static_cast<const char *>(memchr(text + a, '\n', len - a));
        const uint64_t b = lf ? (uint64_t)(lf - text) : len;
        uint64_t e = b;
        if (lf && e > a && text[e - 1] == '\r') e--;   // a CR before the LF
        line++;
        Region r;
        bool skip = false;
        if (!parse_line(text + a, e - a, &r, &skip)) {
            *bad_line = line;
            return false;
        }
        if (!skip) out.push_back(std::move(r));
        a = b + 1;
    }
    return true;
}

inline uint64_t align8(uint64_t x) { return (x + 7) & ~7ull; }

// The table of `regions` (empty ones dropped, a name's intervals sorted and
// merged) into table[0, cap).  ST_E_NOSPACE with *bytes = the size needed;
// ST_E_ARG for a table of 4 GiB or more.
inline int build_table(const std::vector<Region> &regions, uint8_t *table, uint64_t cap, uint64_t *bytes) {
    std::vector<const Region *> live;
    for (const Region &r : regions)
        if (r.start <= r.end) live.push_back(&r);
    std::sort(live.begin(), live.end(), [](const Region *x, const Region *y) {
        if (x->name.size() != y->name.size()) return x->name.size() < y->name.size();
        const int c = memcmp(x->name.data(), y->name.data(), x->name.size());
        if (c) return c < 0;
        return x->start < y->start;
    });
    std::vector<VcfcRegionName> names;
    std::vector<uint64_t> starts, ends;
    std::string nbytes;
    for (size_t i = 0; i < live.size();) {
        size_t j = i;
        VcfcRegionName nm;
        nm.byte_off = (uint32_t)nbytes.size();
        nm.len = (uint32_t)live[i]->name.size();
        nm.iv_first = (uint32_t)starts.size();
        for (; j < live.size() && live[j]->name == live[i]->name; j++) {
            const bool first = j == i;
            // overlapping or adjacent to the last interval: one interval (end + 1 must not wrap)
            if (!first && (ends.back() == UINT64_MAX || live[j]->start <= ends.back() + 1))
                ends.back() = std::max(ends.back(), live[j]->end);
            else {
                starts.push_back(live[j]->start);
                ends.push_back(live[j]->end);
            }
        }
        nm.iv_count = (uint32_t)(starts.size() - nm.iv_first);
        nbytes += live[i]->name;
        names.push_back(nm);
        i = j;
        if (nbytes.size() >= (1ull << 32) || starts.size() >= (1ull << 28)) return ST_E_ARG;
    }
    VcfcRegionsHeader h;
    memset(&h, 0, sizeof h);
    const uint64_t off_names = sizeof h;
    const uint64_t off_starts = align8(off_names + sizeof(VcfcRegionName) * names.size());
    const uint64_t off_ends = off_starts + 8 * starts.size();
    const uint64_t off_bytes = off_ends + 8 * ends.size();
    const uint64_t total = align8(off_bytes + nbytes.size());
    if (total >= (1ull << 32)) return ST_E_ARG;
    *bytes = total;
    if (total > cap || !table) return ST_E_NOSPACE;
    h.magic = VCFC_REGIONS_MAGIC; h.version = VCFC_REGIONS_VERSION;
    h.n_names = (uint32_t)names.size(); h.n_intervals = (uint32_t)starts.size();
    h.off_names = (uint32_t)off_names; h.off_starts = (uint32_t)off_starts; h.off_ends = (uint32_t)off_ends;
    h.off_bytes = (uint32_t)off_bytes; h.total_bytes = (uint32_t)total; h.n_bytes = (uint32_t)nbytes.size();
    memset(table, 0, total);
    memcpy(table, &h, sizeof h);
    if (!names.empty()) memcpy(table + off_names, names.data(), sizeof(VcfcRegionName) * names.size());
    if (!starts.empty()) {
        memcpy(table + off_starts, starts.data(), 8 * starts.size());
        memcpy(table + off_ends, ends.data(), 8 * ends.size());
    }
    if (!nbytes.empty()) memcpy(table + off_bytes, nbytes.data(), nbytes.size());
    return ST_OK;
}

// include/vcfc.h: vcfc_regions_build
inline int regions_build(const char *text, uint64_t len, uint8_t *table, uint64_t cap, uint64_t *bytes, uint64_t *n_regions,
                         uint64_t *bad_line) {
    *bytes = *n_regions = *bad_line = 0;
    std::vector<Region> regions;
    if (!parse_text(text, len, regions, bad_line)) return ST_E_ARG;
    *n_regions = regions.size();
    return build_table(regions, table, cap, bytes);
}

// Everything k_regions_match relies on: the magic word, counts and offsets
// inside `bytes`, the names sorted by (length, bytes) and distinct, every
// name's bytes and intervals inside their arrays, and per name the starts
// ascending with the intervals disjoint.
inline bool regions_validate(const uint8_t *table, uint64_t bytes) {
    VcfcRegionsHeader h;
    if (!table || bytes < sizeof h || bytes >= (1ull << 32)) return false;
    memcpy(&h, table, sizeof h);
    if (h.magic != VCFC_REGIONS_MAGIC || h.version != VCFC_REGIONS_VERSION || h.total_bytes != bytes) return false;
    if ((h.off_names | h.off_starts | h.off_ends) & 7u) return false;
    auto inside = [&](uint64_t off, uint64_t size) { return off >= sizeof h && off <= bytes && size <= bytes - off; };
    if (!inside(h.off_names, sizeof(VcfcRegionName) * (uint64_t)h.n_names) || !inside(h.off_starts, 8ull * h.n_intervals) ||
        !inside(h.off_ends, 8ull * h.n_intervals) || !inside(h.off_bytes, h.n_bytes))
        return false;
    const uint8_t *nb = table + h.off_bytes;
    const uint64_t *starts = reinterpret_cast<const uint64_t *>(table + h.off_starts);
    const uint64_t *ends = reinterpret_cast<const uint64_t *>(table + h.off_ends);
    VcfcRegionName prev;
    memset(&prev, 0, sizeof prev);
    for (uint32_t k = 0; k < h.n_names; k++) {
        VcfcRegionName nm;
        memcpy(&nm, table + h.off_names + sizeof nm * (uint64_t)k, sizeof nm);
        if (nm.byte_off > h.n_bytes || nm.len > h.n_bytes - nm.byte_off) return false;
        if (nm.iv_first > h.n_intervals || nm.iv_count > h.n_intervals - nm.iv_first) return false;
        if (k) {
            if (nm.len < prev.len) return false;
            if (nm.len == prev.len && memcmp(nb + prev.byte_off, nb + nm.byte_off, nm.len) >= 0) return false;
        }
        for (uint32_t j = 0; j < nm.iv_count; j++) {
            const uint64_t a = starts[nm.iv_first + j], b = ends[nm.iv_first + j];
            if (a > b) return false;
            if (j && a <= ends[nm.iv_first + j - 1]) return false;
        }
        prev = nm;
    }
    return true;
}

inline uint64_t regions_workspace_size(uint64_t table_bytes) { return (table_bytes + 255) & ~255ull; }

// include/vcfc.h: vcfc_regions_upload.  The copy has left `table` when the
// call returns.
inline int regions_upload(const uint8_t *table, uint64_t bytes, void *d_ws, uint64_t ws_bytes, hipStream_t s) {
    if (!d_ws || !regions_validate(table, bytes) || ws_bytes < regions_workspace_size(bytes)) return ST_E_ARG;
    if (hipMemcpyAsync(d_ws, table, bytes, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return ST_E_HIP;
    return ST_OK;
}

// include/vcfc.h: vcfc_regions_match_device
inline int regions_match_device(const uint8_t *d_in, const uint64_t *d_rec, uint64_t n, const void *d_ws, uint64_t ws_bytes,
                                uint8_t *d_flag, uint64_t *d_err, hipStream_t s) {
    if ((n && (!d_in || !d_rec || !d_flag)) || !d_ws || ws_bytes < sizeof(VcfcRegionsHeader) || !d_err) return ST_E_ARG;
    return vcfc_regions_match(d_in, d_rec, n, static_cast<const uint8_t *>(d_ws), d_flag, d_err, s) == hipSuccess ? ST_OK
                                                                                                                     : ST_E_HIP;
}

// The match step over a validated host table: prepare uploads it (slot QREF,
// which the one-region step uses for its name), run is k_regions_match.
inline vcfc_dec::MatchStep regions_step(const uint8_t *table, uint64_t bytes, const uint8_t **d_table) {
    vcfc_dec::MatchStep m;
    m.prepare = [=](vcfc_dec::Buffers &B, hipStream_t s) {
        return (*d_table = vcfc_dec::upload(B, vcfc_dec::Buffers::QREF, table, bytes, s)) != nullptr;
    };
    m.run = [=](const uint8_t *d_in, const uint64_t *d_rec, uint64_t nrec, uint8_t *d_flag, uint64_t *d_err, hipStream_t s) {
        return vcfc_regions_match(d_in, d_rec, nrec, *d_table, d_flag, d_err, s);
    };
    return m;
}

}  // namespace vcfc_reg
