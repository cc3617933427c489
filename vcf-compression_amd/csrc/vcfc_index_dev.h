// vcfc_index_dev.h -- device helpers shared by the external-index kernels
// (vcfc_index.hip: binned index; vcfc_sparse_index.hip: sparse index): the
// reference's field parsers restated per record, and the SWAR TAB search.
// Included inside each file's anonymous namespace.
#pragma once

// strtoul(s, &end, 10) with end == s + n required; n == 0 parses as 0
// (str_to_uint64 / str_to_long, reference src/utils.cpp:152-175)
__device__ __forceinline__ bool idx_strtoul(const uint8_t *s, uint64_t n, uint64_t *out) {
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
        ovf = ovf || v > (~0ull - d) / 10;
        v = v * 10 + d;
    }
    if (i != n) return false;
    *out = ovf ? ~0ull : (neg ? 0ull - v : v);
    return true;
}

// reference_name_map (src/utils.hpp:97-100): "1".."22", "X", "Y", "M" -> 1..25, else 0
__device__ __forceinline__ uint32_t idx_ref(const uint8_t *c, uint64_t n) {
    if (n == 1) {
        if (c[0] >= '1' && c[0] <= '9') return (uint32_t)(c[0] - '0');
        return c[0] == 'X' ? 23u : c[0] == 'Y' ? 24u : c[0] == 'M' ? 25u : 0u;
    }
    if (n == 2) {
        if (c[0] == '1' && c[1] >= '0' && c[1] <= '9') return 10u + (uint32_t)(c[1] - '0');
        if (c[0] == '2' && c[1] >= '0' && c[1] <= '2') return 20u + (uint32_t)(c[1] - '0');
    }
    return 0;
}

// ALT without '<': the longest non-empty ','-piece (0 if none); *sv = a '<' seen
__device__ __forceinline__ uint64_t idx_alt_longest(const uint8_t *a, uint64_t n, bool *sv) {
    uint64_t best = 0, run = 0;
    bool lt = false;
    for (uint64_t k = 0; k < n; k++) {
        const uint8_t c = a[k];
        lt = lt || c == '<';
        run = c == ',' ? 0 : run + 1;
        best = run > best ? run : best;
    }
    *sv = lt;
    return best;
}

// max over the non-empty ','-pieces of v[0, n) of (long)strtoul(piece), or of
// its magnitude (SVLEN); signed compares from 0 as the reference's
__device__ __forceinline__ bool idx_list_max(const uint8_t *v, uint64_t n, bool magnitude, int64_t *out) {
    int64_t best = 0;
    uint64_t k = 0;
    while (k < n) {
        uint64_t e = k;
        while (e < n && v[e] != ',') e++;
        if (e > k) {
            uint64_t u = 0;
            if (!idx_strtoul(v + k, e - k, &u)) return false;
            int64_t x = (int64_t)u;
            if (magnitude && x < 0) x = (int64_t)(0ull - u);   // std::abs (LONG_MIN stays)
            if (x > best) best = x;
        }
        k = e + 1;
    }
    *out = best;
    return true;
}

// compute_end_position for a structural ALT: parse_kvp over INFO (pairs on
// ';', parts on '=', empty pieces dropped; a pair with other than 1 or 2
// parts throws; later keys overwrite), then END, else SVLEN, else pos
__device__ bool idx_sv_end(const uint8_t *info, uint64_t n, uint64_t pos, uint64_t *end) {
    bool has_end = false, has_svlen = false;
    uint64_t ev = 0, en = 0, sv = 0, sn = 0;
    uint64_t k = 0;
    while (k < n) {
        uint64_t pe = k;
        while (pe < n && info[pe] != ';') pe++;
        if (pe > k) {
            uint32_t parts = 0;
            uint64_t k0 = 0, n0 = 0, k1 = 0, n1 = 0;
            uint64_t q = k;
            while (q < pe) {
                uint64_t qe = q;
                while (qe < pe && info[qe] != '=') qe++;
                if (qe > q) {
                    if (parts == 0) { k0 = q; n0 = qe - q; }
                    else if (parts == 1) { k1 = q; n1 = qe - q; }
                    parts++;
                }
                q = qe + 1;
            }
            if (parts != 1 && parts != 2) return false;
            if (parts == 1) { k1 = 0; n1 = 0; }
            const uint8_t *key = info + k0;
            if (n0 == 3 && key[0] == 'E' && key[1] == 'N' && key[2] == 'D') { has_end = true; ev = k1; en = n1; }
            if (n0 == 5 && key[0] == 'S' && key[1] == 'V' && key[2] == 'L' && key[3] == 'E' && key[4] == 'N') {
                has_svlen = true; sv = k1; sn = n1;
            }
        }
        k = pe + 1;
    }
    int64_t m = 0;
    if (has_end) {
        if (!idx_list_max(info + ev, en, false, &m)) return false;
        *end = (uint64_t)m;
    } else if (has_svlen) {
        if (!idx_list_max(info + sv, sn, true, &m)) return false;
        *end = pos + (uint64_t)m - 1;
    } else {
        *end = pos;
    }
    return true;
}

// 0x80 in every byte of x that is a TAB (exact per byte)
__device__ __forceinline__ uint32_t tab_z(uint32_t x) {
    const uint32_t t = x ^ 0x09090909u;
    return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
}
__device__ __forceinline__ uint64_t tab_bits16(uint4 v) {
    auto b4 = [](uint32_t z) { return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u); };
    return (uint64_t)(b4(tab_z(v.x)) | b4(tab_z(v.y)) << 4 | b4(tab_z(v.z)) << 8 | b4(tab_z(v.w)) << 12);
}

// `need` more TABs in in[k, re)?  16-byte loads while they fit below re.
__device__ __forceinline__ bool idx_more_tabs(const uint8_t *in, uint64_t k, uint64_t re, uint32_t need) {
    while (need && k + 16 <= re) {
        const uint4 v = vw::uload16(in + k);
        const uint32_t c = (uint32_t)vw::popc64((uint64_t)tab_z(v.x) | (uint64_t)tab_z(v.y) << 32) +
                           (uint32_t)vw::popc64((uint64_t)tab_z(v.z) | (uint64_t)tab_z(v.w) << 32);
        need = c >= need ? 0 : need - c;
        k += 16;
    }
    for (; need && k < re; k++)
        if (in[k] == '\t') need--;
    return need == 0;
}
