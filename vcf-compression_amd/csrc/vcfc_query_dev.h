// vcfc_query_dev.h -- device code shared by the kernels that match records
// against coordinates: k_query_match (vcfc_decode.hip, one region) and
// k_regions_match (vcfc_regions.hip, a region table).  Both run one lane per
// record through query_frame: it finds CHROM and POS, parses POS and reports
// the match errors; the kernels differ only in the verdict they pass in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// strtoul(s, &end, 10) with end == s + n required; n == 0 parses as 0
__device__ __forceinline__ bool pos_parse(const uint8_t *s, uint64_t n, uint64_t *out) {
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

// CHROM and POS of the record at p (CHROM starts at p + 8): *f1 = POS start,
// *f2 = the TAB after POS (both TABs searched below lim)
__device__ __forceinline__ bool query_fields(const uint8_t *in, uint64_t p, uint64_t lim, uint64_t *f1, uint64_t *f2) {
    uint64_t k = p + 8;
    while (k < lim && in[k] != '\t') k++;
    if (k >= lim) return false;
    *f1 = ++k;
    while (k < lim && in[k] != '\t') k++;
    if (k >= lim) return false;
    *f2 = k;
    return true;
}

// bit j of the result: byte j of x is a TAB (exact per byte)
__device__ __forceinline__ uint32_t tab_bits(uint32_t x) {
    const uint32_t t = x ^ 0x09090909u;
    const uint32_t z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);   // 0x80 in each zero byte
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

// One lane per record.  Fast path: the 32 bytes from the 16-byte block
// holding the CHROM start lie inside the record; two 16-byte loads, TABs
// found by SWAR in registers, the fields parsed from an LDS copy.  Otherwise
// (CHROM + POS longer than the window holds) byte by byte.  (32 bytes hold
// "22\t" + a 9-digit POS + TAB from any of the 16 phases; round 6: 48 -> 32,
// one load and ~13 % of the cache lines fewer per record.)
// win: the block's 256 * QM_WIN bytes of LDS.  matches(name, name_len, pos)
// is the verdict for a record whose POS parsed; name points into the LDS
// copy on the fast path, into `in` otherwise.
constexpr uint32_t QM_WIN = 32;
template <class Matches>
__device__ __forceinline__ void query_frame(const uint8_t *in, const uint64_t *rec, uint64_t n, uint8_t *win,
                                            uint8_t *flag, uint64_t *err, Matches &&matches) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t rs = rec[i], re = rec[i + 1];
    const uint8_t *p = in + rs + 8;
    const uint8_t *a = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(p) & ~(uintptr_t)15);
    uint64_t f1 = 0, f2 = 0, pos = 0;
    uint32_t code = 0;
    bool m = false, done = false;
    if (a + QM_WIN <= in + re) {
        const uint4 *g = reinterpret_cast<const uint4 *>(a);
        const uint4 v0 = g[0], v1 = g[1];
        uint4 *w = reinterpret_cast<uint4 *>(win + threadIdx.x * QM_WIN);
        w[0] = v0; w[1] = v1;
        const uint64_t tabs = (uint64_t)tab_bits(v0.x) | (uint64_t)tab_bits(v0.y) << 4 | (uint64_t)tab_bits(v0.z) << 8 |
                              (uint64_t)tab_bits(v0.w) << 12 | (uint64_t)tab_bits(v1.x) << 16 |
                              (uint64_t)tab_bits(v1.y) << 20 | (uint64_t)tab_bits(v1.z) << 24 |
                              (uint64_t)tab_bits(v1.w) << 28;
        const uint32_t sh = (uint32_t)(p - a);
        const uint64_t t = tabs >> sh;
        const uint64_t t2 = t & (t - 1);
        if (t2) {   // both TABs inside the window
            const uint32_t c = (uint32_t)__builtin_ctzll(t), d = (uint32_t)__builtin_ctzll(t2);
            const uint8_t *f = win + threadIdx.x * QM_WIN + sh;
            if (!pos_parse(f + c + 1, d - c - 1, &pos)) code = 2;
            else m = matches(f, (uint64_t)c, pos);
            done = true;
        }
    }
    if (!done) {
        if (!query_fields(in, rs, re, &f1, &f2)) code = 3;
        else if (!pos_parse(in + f1, f2 - f1, &pos)) code = 2;
        else m = matches(in + rs + 8, f1 - 1 - (rs + 8), pos);
    }
    flag[i] = m ? 1 : 0;
    if (code) atomicMin((unsigned long long *)err, (unsigned long long)((i << 8) | code));
}

}  // namespace
