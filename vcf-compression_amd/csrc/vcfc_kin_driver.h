// vcfc_kin_driver.h -- host driver of kinship, shared by the C
// ABI (vcfc_api.cpp) and the CPU emulator harness
// (tests/simt_emu/emu_kin_api.cpp), so the same control flow is tested on both.
//
//   1. the header and vcfc_dec::open_section, as genotype-matrix: record
//      starts, and with a query the flags of the records that are rows;
//   2. the records in batches whose workspace (.bed rows, bit planes, the
//      matrix call's: batch_need) fits ws_bound: one composed device call (rows, planes,
//      pairs) a batch into one square on the device; the first batch stores,
//      the later ones accumulate -- tables are additive over rows;
//   3. a selected record that is not regular ends the rows: the device call
//      counts the rows before it only, so the square is that of the rows
//      before it, as if the file ended there; ST_E_FORMAT then, at a match
//      error, or where hopping stopped with 8 or more bytes left.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vcfc_matrix_driver.h"

namespace vcfc_kin {

using vcfc_cnt::Query;
using vcfc_dec::Buffers;
using vcfc_gm::ST_OK;
using vcfc_gm::ST_E_ARG;
using vcfc_gm::ST_E_HIP;
using vcfc_gm::ST_E_FORMAT;

struct Result {
    std::vector<uint64_t> index;     // file index of each row's record
    std::vector<uint32_t> tables;    // S x S x 9
    uint64_t err_record = ~0ull;     // the record the call stopped at
};

inline bool shape_ok(uint64_t n, uint64_t S) {
    // n < 2^32 as the matrix call, so a cell fits 32 bits; S < 2^30 as the matrix call
    return S != 0 && S < (1ull << 30) && n < (1ull << 32);
}

inline void args_workspace(VcfcKinArgs &a, uint8_t *ws, const VcfcKinLayout &L) {
    a.state = reinterpret_cast<uint64_t *>(ws + L.state);
    a.planes = reinterpret_cast<uint32_t *>(ws + L.planes);
    a.row_words = L.row_words;
}

// The pair step alone (include/vcfc.h: vcfc_kin_tables_device).
inline int tables_device(const uint8_t *d_bed, uint64_t n_rows, uint64_t row_stride, uint64_t S, uint32_t *d_tables,
                         uint64_t tables_cap, int accumulate, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, hipStream_t s) {
    if ((n_rows && !d_bed) || !d_tables || !d_ws || !d_err || !shape_ok(n_rows, S) || tables_cap < S * S) return ST_E_ARG;
    if (row_stride < vcfc_matrix_row_size(VCFC_MATRIX_BED, S)) return ST_E_ARG;
    const VcfcKinLayout L = vcfc_kin_workspace_layout(n_rows, S);
    if (ws_bytes < L.total) return ST_E_ARG;
    VcfcKinArgs a;
    a.bed = d_bed; a.row_stride = row_stride; a.n = n_rows; a.row_of = nullptr; a.S = S; a.tables = d_tables;
    a.accumulate = accumulate; a.err = d_err; a.own_err = true;
    args_workspace(a, static_cast<uint8_t *>(d_ws), L);
    return vcfc_kin_run(a, s) == hipSuccess ? ST_OK : ST_E_HIP;
}

// The composed call (include/vcfc.h: vcfc_kin_records_device): the matrix call
// writes the .bed rows into the workspace, then planes and pairs.
inline int records_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec, const uint8_t *d_select, uint64_t n,
                          uint64_t S, uint32_t *d_tables, uint64_t tables_cap, int accumulate, uint64_t *d_row_of, void *d_ws,
                          uint64_t ws_bytes, uint64_t *d_err, hipStream_t s) {
    if ((n && (!d_in || !d_rec)) || !d_tables || !d_row_of || !d_ws || !d_err || !shape_ok(n, S) || tables_cap < S * S)
        return ST_E_ARG;
    const VcfcKinLayout L = vcfc_kin_workspace_layout(n, S);
    if (ws_bytes < L.total) return ST_E_ARG;
    uint8_t *ws = static_cast<uint8_t *>(d_ws);
    const int st = vcfc_gm::matrix_device(d_in, in_bytes, d_rec, d_select, n, S, VCFC_MATRIX_BED, ws + L.bed, L.bed_stride * n,
                                          L.bed_stride, d_row_of, ws + L.matrix, L.total - L.matrix, d_err, s);
    if (st != ST_OK) return st;
    VcfcKinArgs a;
    a.bed = ws + L.bed; a.row_stride = L.bed_stride; a.n = n; a.row_of = d_row_of; a.S = S; a.tables = d_tables;
    a.accumulate = accumulate; a.err = d_err; a.own_err = false;
    args_workspace(a, ws, L);
    return vcfc_kin_run(a, s) == hipSuccess ? ST_OK : ST_E_HIP;
}

// bytes a batch of n records needs in the workspace: planes, .bed rows and the matrix call's part, before the
// layout's alignment (so it grows with every record and a bound names a record count exactly)
inline uint64_t batch_need(uint64_t n, uint64_t S) {
    const VcfcKinLayout L = vcfc_kin_workspace_layout(n, S);
    return 12 * L.row_words * S + L.bed_stride * n + vcfc_matrix_workspace_layout(n).total;
}

// records per batch: the most that need at most ws_bound bytes (256 MiB where the caller names none), at least 1
inline uint64_t batch_records(uint64_t S, uint64_t ws_bound) {
    if (!ws_bound) ws_bound = 256ull << 20;
    uint64_t lo = 1, hi = 1ull << 22;   // (the matrix driver's cap)
    if (batch_need(hi, S) <= ws_bound) return hi;
    while (hi - lo > 1) {   // lo fits or is 1; hi does not fit
        const uint64_t mid = lo + (hi - lo) / 2;
        (batch_need(mid, S) <= ws_bound ? lo : hi) = mid;
    }
    return lo;
}

// The data section of a .vcfc (host bytes h_in[0, n); uploaded here).  q ==
// nullptr: every record is a row; else the records the match step flags.
inline int kin_section(const uint8_t *h_in, uint64_t n, uint64_t S, const vcfc_dec::MatchStep *q, Buffers &B, hipStream_t s,
                       Result &R, uint64_t ws_bound = 0) {
    R = Result();
    if (!shape_ok(0, S)) return ST_E_ARG;
    vcfc_dec::Section X;
    std::vector<uint8_t> flag;
    const int st = vcfc_dec::open_section(h_in, n, q, B, s, X, &flag);
    if (st) return st;
    const uint64_t k = X.k, batch = batch_records(S, ws_bound), cells = S * S * 9;
    uint32_t *d_tables = static_cast<uint32_t *>(B.get(Buffers::OUT, 4 * cells + 64));
    if (!d_tables) return ST_E_HIP;
    if (k == 0 && hipMemsetAsync(d_tables, 0, 4 * cells, s) != hipSuccess) return ST_E_HIP;
    bool failed = false;
    for (uint64_t i0 = 0; i0 < k && !failed; i0 += batch) {
        const uint64_t nb = std::min(batch, k - i0);
        const VcfcKinLayout L = vcfc_kin_workspace_layout(nb, S);
        void *ws = B.get(Buffers::WS, L.total);
        uint64_t *d_row_of = static_cast<uint64_t *>(B.get(Buffers::LINE_OFF, 8 * (nb + 1)));
        if (!ws || !d_row_of) return ST_E_HIP;
        uint64_t err = 0;
        if (records_device(X.d_in, n, X.d_rec + i0, X.d_flag ? X.d_flag + i0 : nullptr, nb, S, d_tables, S * S, i0 != 0, d_row_of,
                           ws, L.total, X.d_small, s) != ST_OK ||
            hipMemcpyAsync(&err, X.d_small, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
        uint64_t good = nb;
        if (err != VCFCD_NO_ERROR) {
            if ((err & 0xFF) != 3) return ST_E_HIP;   // (the rows were sized for the records)
            good = err >> 8;   // record i0 + good is not regular: the device counted the rows before it
            R.err_record = i0 + good;
            failed = true;
        }
        for (uint64_t j = 0; j < good; j++)
            if (!q || flag[i0 + j]) R.index.push_back(i0 + j);
    }
    R.tables.resize(cells);
    if (hipMemcpyAsync(R.tables.data(), d_tables, 4 * cells, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return ST_E_HIP;
    if (failed) return ST_E_FORMAT;
    if (k < X.nrec || X.tail()) {
        R.err_record = k;
        return ST_E_FORMAT;
    }
    return ST_OK;
}

// A whole .vcfc: header, then kin_section.
inline int kin_file(const uint8_t *in, uint64_t n, const vcfc_dec::MatchStep *match, Buffers &B, hipStream_t s, Result &R,
                    uint64_t *data_off, uint64_t *S, uint64_t ws_bound = 0) {
    R = Result();
    const int st = vcfc_cnt::counts_header(in, n, data_off, S);
    if (st) return st;
    return kin_section(in + *data_off, n - *data_off, *S, match, B, s, R, ws_bound);
}

// kin_file with one region (q == nullptr: every record)
inline int kin_file(const uint8_t *in, uint64_t n, const Query *q, Buffers &B, hipStream_t s, Result &R, uint64_t *data_off,
                    uint64_t *S, uint64_t ws_bound = 0) {
    R = Result();
    if (!q) return kin_file(in, n, static_cast<const vcfc_dec::MatchStep *>(nullptr), B, s, R, data_off, S, ws_bound);
    VcfcQuery vq;
    const vcfc_dec::MatchStep match = vcfc_dec::region_step(q->ref, q->ref_len, q->has_range, q->start, q->end, &vq);
    const int st = vcfc_cnt::counts_header(in, n, data_off, S);
    if (st) return st;
    if (q->ref_len > 0xFFFFFFFFull) return ST_E_FORMAT;
    return kin_section(in + *data_off, n - *data_off, *S, &match, B, s, R, ws_bound);
}

// The statistics of a table: integers exact in 64 bits, then
// one conversion per operand and one division in double.
struct Stats {
    uint64_t N, ibs0, ibs1, ibs2, hh, het_a, het_b;
    bool has_dst, has_kin;
    double dst, kin;
};
inline Stats table_stats(const uint32_t *t) {
    Stats x;
    x.N = 0;
    for (int e = 0; e < 9; e++) x.N += t[e];
    x.ibs0 = (uint64_t)t[2] + t[6];
    x.ibs2 = (uint64_t)t[0] + t[4] + t[8];
    x.ibs1 = x.N - x.ibs0 - x.ibs2;
    x.hh = t[4];
    x.het_a = (uint64_t)t[3] + t[4] + t[5];
    x.het_b = (uint64_t)t[1] + t[4] + t[7];
    const uint64_t m = std::min(x.het_a, x.het_b);
    x.has_dst = x.N != 0;
    x.has_kin = m != 0;
    x.dst = x.has_dst ? (double)(int64_t)(2 * x.ibs2 + x.ibs1) / (double)(int64_t)(2 * x.N) : 0.0;
    const int64_t num = 2 * (int64_t)x.hh - 4 * (int64_t)x.ibs0 + 2 * (int64_t)m - (int64_t)x.het_a - (int64_t)x.het_b;
    x.kin = x.has_kin ? (double)num / (double)(int64_t)(4 * m) : 0.0;
    return x;
}

// The pairs as text: the header line, then per written pair i < j the two
// sample names from the '#CHROM' line (in: the file, data_off: its data
// section), the seven integers, DST and KINSHIP.
inline void render_tsv(const uint8_t *in, uint64_t data_off, uint64_t S, const Result &R, bool has_min, double min_kinship,
                       std::vector<uint8_t> &out) {
    static const char head[] = "#ID_A\tID_B\tN\tIBS0\tIBS1\tIBS2\tHETHET\tHET_A\tHET_B\tDST\tKINSHIP\n";
    out.assign(head, head + sizeof head - 1);
    std::vector<uint64_t> f;
    vcfc_sub::header_fields(in, data_off, f);   // S + 9 fields
    char num[256];
    for (uint64_t i = 0; i < S; i++)
        for (uint64_t j = i + 1; j < S; j++) {
            const Stats x = table_stats(R.tables.data() + (i * S + j) * 9);
            if (has_min && !(x.has_kin && x.kin >= min_kinship)) continue;
            out.insert(out.end(), in + f[9 + i], in + f[10 + i] - 1);
            out.push_back('\t');
            out.insert(out.end(), in + f[9 + j], in + f[10 + j] - 1);
            int len = snprintf(num, sizeof num, "\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t", (unsigned long long)x.N,
                               (unsigned long long)x.ibs0, (unsigned long long)x.ibs1, (unsigned long long)x.ibs2,
                               (unsigned long long)x.hh, (unsigned long long)x.het_a, (unsigned long long)x.het_b);
            len += x.has_dst ? snprintf(num + len, sizeof num - len, "%.6g\t", x.dst) : snprintf(num + len, sizeof num - len, "nan\t");
            len += x.has_kin ? snprintf(num + len, sizeof num - len, "%.6g\n", x.kin) : snprintf(num + len, sizeof num - len, "nan\n");
            out.insert(out.end(), num, num + len);
        }
}

}  // namespace vcfc_kin
