// vcfc_ld_driver.h -- host driver of ld-window, shared by the
// C ABI (vcfc_api.cpp) and the CPU emulator harness
// (tests/simt_emu/emu_ld_api.cpp), so the same control flow is tested on both.
//
//   1. the header and vcfc_dec::open_section, as genotype-matrix: record
//      starts, and with a query the flags of the records that are rows;
//   2. the rows in batches whose band (owned rows x W tables) fits band_bound:
//      a batch is the records of its owned rows and of a halo of W rows after
//      them, so a pair that spans a batch end is computed once, by the batch
//      that owns its row i; one composed device call (rows, planes, pairs) a
//      batch, the owned rows' tables copied back;
//   3. a selected record that is not regular ends the rows: its batch runs
//      once more without it, so the band is that of the rows before it, as if
//      the file ended there; ST_E_FORMAT then, at a match error, or where
//      hopping stopped with 8 or more bytes left.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vcfc_matrix_driver.h"

namespace vcfc_ld {

using vcfc_cnt::Query;
using vcfc_dec::Buffers;
using vcfc_gm::ST_OK;
using vcfc_gm::ST_E_ARG;
using vcfc_gm::ST_E_HIP;
using vcfc_gm::ST_E_FORMAT;

struct Result {
    std::vector<uint64_t> index;     // file index of each row's record
    std::vector<uint32_t> tables;    // rows x W x 9
    uint64_t err_record = ~0ull;     // the record the call stopped at
    std::vector<uint64_t> rec_start; // the hopped records' offsets in the data section
};

inline bool shape_ok(uint64_t n, uint64_t S, uint64_t W) {
    // n < 2^32 as the matrix call; S < 2^30: a cell fits 32 bits, r2's integers 64; W < 2^16: the partner tiles are gridDim.y
    return W != 0 && W < (1ull << 16) && S != 0 && S < (1ull << 30) && n < (1ull << 32);
}

inline void args_workspace(VcfcLdArgs &a, uint8_t *ws, const VcfcLdLayout &L) {
    a.state = reinterpret_cast<uint64_t *>(ws + L.state);
    a.planes = reinterpret_cast<uint32_t *>(ws + L.planes);
    a.plane_words = L.plane_words;
}

// The pair step alone (include/vcfc.h: vcfc_ld_tables_device).
inline int tables_device(const uint8_t *d_bed, uint64_t n_rows, uint64_t row_stride, uint64_t S, uint64_t W, uint32_t *d_tables,
                         uint64_t pairs_cap, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, hipStream_t s) {
    if ((n_rows && !d_bed) || !d_tables || !d_ws || !d_err || !shape_ok(n_rows, S, W)) return ST_E_ARG;
    if (row_stride < vcfc_matrix_row_size(VCFC_MATRIX_BED, S)) return ST_E_ARG;
    const VcfcLdLayout L = vcfc_ld_workspace_layout(n_rows, S);
    if (ws_bytes < L.total) return ST_E_ARG;
    VcfcLdArgs a;
    a.bed = d_bed; a.row_stride = row_stride; a.n = n_rows; a.rows_dev = nullptr; a.select = nullptr; a.row_of = nullptr;
    a.S = S; a.W = W; a.tables = d_tables; a.pairs_cap = pairs_cap; a.err = d_err; a.own_err = true;
    args_workspace(a, static_cast<uint8_t *>(d_ws), L);
    return vcfc_ld_run(a, s) == hipSuccess ? ST_OK : ST_E_HIP;
}

// The composed call (include/vcfc.h: vcfc_ld_window_device): the matrix call
// writes the .bed rows into the workspace, then planes and pairs.
inline int window_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec, const uint8_t *d_select, uint64_t n,
                         uint64_t S, uint64_t W, uint32_t *d_tables, uint64_t pairs_cap, uint64_t *d_row_of, void *d_ws,
                         uint64_t ws_bytes, uint64_t *d_err, hipStream_t s) {
    if ((n && (!d_in || !d_rec)) || !d_tables || !d_row_of || !d_ws || !d_err || !shape_ok(n, S, W)) return ST_E_ARG;
    const VcfcLdLayout L = vcfc_ld_workspace_layout(n, S);
    if (ws_bytes < L.total) return ST_E_ARG;
    uint8_t *ws = static_cast<uint8_t *>(d_ws);
    const int st = vcfc_gm::matrix_device(d_in, in_bytes, d_rec, d_select, n, S, VCFC_MATRIX_BED, ws + L.bed, L.bed_stride * n,
                                          L.bed_stride, d_row_of, ws + L.matrix, L.total - L.matrix, d_err, s);
    if (st != ST_OK) return st;
    VcfcLdArgs a;
    a.bed = ws + L.bed; a.row_stride = L.bed_stride; a.n = n; a.rows_dev = d_row_of + n; a.select = d_select; a.row_of = d_row_of;
    a.S = S; a.W = W; a.tables = d_tables; a.pairs_cap = pairs_cap; a.err = d_err; a.own_err = false;
    args_workspace(a, ws, L);
    return vcfc_ld_run(a, s) == hipSuccess ? ST_OK : ST_E_HIP;
}

// owned rows per batch: a band of at most band_bound bytes (256 MiB where the caller names none)
inline uint64_t batch_rows(uint64_t W, uint64_t band_bound) {
    if (!band_bound) band_bound = 256ull << 20;
    return std::max<uint64_t>(1, band_bound / (36 * W));
}

// The data section of a .vcfc (host bytes h_in[0, n); uploaded here).  q ==
// nullptr: every record is a row; else the records the match step flags.
inline int window_section(const uint8_t *h_in, uint64_t n, uint64_t S, uint64_t W, const vcfc_dec::MatchStep *q, Buffers &B,
                          hipStream_t s, Result &R, uint64_t band_bound = 0) {
    R = Result();
    if (!shape_ok(0, S, W)) return ST_E_ARG;
    vcfc_dec::Section X;
    std::vector<uint8_t> flag;
    const int st = vcfc_dec::open_section(h_in, n, q, B, s, X, &flag);
    R.rec_start = X.rec;
    if (st) return st;
    std::vector<uint64_t> &sel = R.index;   // the records that are rows, while none of them has failed
    for (uint64_t i = 0; i < X.k; i++)
        if (!q || flag[i]) sel.push_back(i);
    const uint64_t own = batch_rows(W, band_bound);
    bool failed = false;
    for (uint64_t r0 = 0; r0 < sel.size();) {
        const uint64_t owned = std::min<uint64_t>(own, sel.size() - r0);
        const uint64_t last = std::min<uint64_t>(sel.size(), r0 + owned + W) - 1;   // the halo's last row
        const uint64_t a = sel[r0], nb = sel[last] + 1 - a, rows = last + 1 - r0;
        const VcfcLdLayout L = vcfc_ld_workspace_layout(nb, S);
        void *ws = B.get(Buffers::WS, L.total);
        uint32_t *d_tables = static_cast<uint32_t *>(B.get(Buffers::OUT, rows * W * 36 + 64));
        uint64_t *d_row_of = static_cast<uint64_t *>(B.get(Buffers::LINE_OFF, 8 * (nb + 1)));
        if (!ws || !d_tables || !d_row_of) return ST_E_HIP;
        uint64_t err = 0;
        if (window_device(X.d_in, n, X.d_rec + a, X.d_flag ? X.d_flag + a : nullptr, nb, S, W, d_tables, rows * W, d_row_of, ws,
                          L.total, X.d_small, s) != ST_OK ||
            hipMemcpyAsync(&err, X.d_small, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
        if (err != VCFCD_NO_ERROR) {
            if ((err & 0xFF) != 3) return ST_E_HIP;   // (the band was sized for the rows)
            // record a + (err >> 8) is not regular: the rows end before it, and the batch runs again without it
            R.err_record = a + (err >> 8);
            failed = true;
            sel.resize(std::lower_bound(sel.begin(), sel.end(), R.err_record) - sel.begin());
            continue;
        }
        const uint64_t have = R.tables.size();
        R.tables.resize(have + owned * W * 9);
        if (hipMemcpyAsync(R.tables.data() + have, d_tables, owned * W * 36, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
        r0 += owned;
    }
    if (failed) return ST_E_FORMAT;
    if (X.k < X.nrec || X.tail()) {
        R.err_record = X.k;
        return ST_E_FORMAT;
    }
    return ST_OK;
}

// A whole .vcfc: header, then window_section.
inline int window_file(const uint8_t *in, uint64_t n, uint64_t W, const vcfc_dec::MatchStep *match, Buffers &B, hipStream_t s,
                       Result &R, uint64_t *data_off, uint64_t *S, uint64_t band_bound = 0) {
    R = Result();
    if (W == 0 || W >= (1ull << 16)) return ST_E_ARG;
    const int st = vcfc_cnt::counts_header(in, n, data_off, S);
    if (st) return st;
    return window_section(in + *data_off, n - *data_off, *S, W, match, B, s, R, band_bound);
}

// window_file with one region (q == nullptr: every record)
inline int window_file(const uint8_t *in, uint64_t n, uint64_t W, const Query *q, Buffers &B, hipStream_t s, Result &R,
                       uint64_t *data_off, uint64_t *S, uint64_t band_bound = 0) {
    R = Result();
    if (!q) return window_file(in, n, W, static_cast<const vcfc_dec::MatchStep *>(nullptr), B, s, R, data_off, S, band_bound);
    if (W == 0 || W >= (1ull << 16)) return ST_E_ARG;
    VcfcQuery vq;
    const vcfc_dec::MatchStep match = vcfc_dec::region_step(q->ref, q->ref_len, q->has_range, q->start, q->end, &vq);
    const int st = vcfc_cnt::counts_header(in, n, data_off, S);
    if (st) return st;
    if (q->ref_len > 0xFFFFFFFFull) return ST_E_FORMAT;
    return window_section(in + *data_off, n - *data_off, *S, W, &match, B, s, R, band_bound);
}

// r2 of a table: integers exact in 64 bits (S < 2^30), then
// three conversions, two multiplications and one division in double; false
// where it is undefined.  *N: the table's sum.
inline bool table_r2(const uint32_t *t, uint64_t *N, double *r2) {
    int64_t n = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const int64_t c = t[3 * a + b];
            n += c; sx += a * c; sy += b * c; sxx += a * a * c; syy += b * b * c; sxy += a * b * c;
        }
    *N = (uint64_t)n;
    const int64_t cov = n * sxy - sx * sy, vx = n * sxx - sx * sx, vy = n * syy - sy * sy;
    if (vx == 0 || vy == 0) return false;
    const double c = (double)cov, x = (double)vx, y = (double)vy;
    const double num = c * c, den = x * y;
    *r2 = num / den;
    return true;
}

// The pairs as text (data: the file's data section; a regular record has 9
// TABs inside REQ): the header line, then per written pair, in slot order,
// CHROM POS ID of both records, N and r2.
inline void render_tsv(const uint8_t *data, const Result &R, uint64_t W, double min_r2, std::vector<uint8_t> &out) {
    static const char head[] = "#CHROM_A\tPOS_A\tID_A\tCHROM_B\tPOS_B\tID_B\tN\tR2\n";
    out.assign(head, head + sizeof head - 1);
    const uint64_t rows = R.index.size();
    auto fields = [&](uint64_t r, uint64_t *f) {   // ends of fields 0..2 (their TABs), from REQ's start
        const uint8_t *p = data + R.rec_start[R.index[r]] + 8;
        for (uint64_t e = 0, k = 0; k < 3; e++)
            if (p[e] == '\t') f[k++] = e;
        return p;
    };
    char num[64];
    for (uint64_t i = 0; i < rows; i++) {
        uint64_t fa[3], fb[3];
        const uint8_t *pa = fields(i, fa);
        for (uint64_t k = 1; k <= W && i + k < rows; k++) {
            const uint8_t *pb = fields(i + k, fb);
            if (fa[0] != fb[0] || memcmp(pa, pb, fa[0]) != 0) continue;
            uint64_t N = 0;
            double r2 = 0;
            const bool defined = table_r2(R.tables.data() + (i * W + k - 1) * 9, &N, &r2);
            if (min_r2 > 0 && !(defined && r2 >= min_r2)) continue;
            out.insert(out.end(), pa, pa + fa[2] + 1);
            out.insert(out.end(), pb, pb + fb[2] + 1);
            const int len = defined ? snprintf(num, sizeof num, "%llu\t%.6g\n", (unsigned long long)N, r2)
                                    : snprintf(num, sizeof num, "%llu\tnan\n", (unsigned long long)N);
            out.insert(out.end(), num, num + len);
        }
    }
}

}  // namespace vcfc_ld
