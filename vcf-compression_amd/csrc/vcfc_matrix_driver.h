// vcfc_matrix_driver.h -- host driver of genotype-matrix,
// shared by the C ABI (vcfc_api.cpp) and the CPU emulator harness
// (tests/simt_emu/emu_matrix_api.cpp), so the same control flow is tested on
// both.
//
//   1. the header: S from the '#CHROM' line (ST_E_ARG for S == 0 or >= 2^30);
//   2. vcfc_dec::open_section: record starts, and with a query the flags of
//      the records that get a row, on the host too;
//   3. the records in batches of rec_batch: one pass each writes the batch's
//      rows densely on the device;
//   4. ST_E_FORMAT at the first selected record that is not regular, at a
//      match error, or where hopping stopped with 8 or more bytes left: the
//      rows before it are kept.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "vcfc_counts_driver.h"
#include "vcfc_decode_driver.h"
#include "vcfc_device.h"
#include "vcfc_subset_driver.h"

namespace vcfc_gm {

using vcfc_cnt::Query;
using vcfc_dec::Buffers;
constexpr int ST_OK = 0, ST_E_ARG = 5, ST_E_HIP = 6, ST_E_IO = 7, ST_E_FORMAT = 8;   // = include/vcfc.h codes

struct Result {
    std::vector<uint64_t> index;     // file index of each row's record
    std::vector<uint8_t> rows;       // row_bytes per row, dense
    uint64_t err_record = ~0ull;     // the record the call stopped at
    std::vector<uint64_t> rec_start; // the hopped records' offsets in the data section
};

// The device entry (include/vcfc.h: vcfc_genotype_matrix_device): argument
// checks, then the kernels enqueued on s.
inline int matrix_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec, const uint8_t *d_select, uint64_t n,
                         uint64_t S, int layout, uint8_t *d_out, uint64_t out_cap, uint64_t row_stride, uint64_t *d_row_of,
                         void *d_ws, uint64_t ws_bytes, uint64_t *d_err, hipStream_t s) {
    if ((n && (!d_in || !d_rec)) || !d_out || !d_row_of || !d_ws || !d_err) return ST_E_ARG;
    if (layout != VCFC_MATRIX_DOSAGE && layout != VCFC_MATRIX_HAP && layout != VCFC_MATRIX_BED) return ST_E_ARG;
    // n < 2^32: the queue holds 32-bit indices; S < 2^30: a row's bytes and a window's token count stay 32-bit
    if (S == 0 || S >= (1ull << 30) || n >= (1ull << 32) || row_stride < vcfc_matrix_row_size(layout, S)) return ST_E_ARG;
    const VcfcMatrixLayout L = vcfc_matrix_workspace_layout(n);
    if (ws_bytes < L.total) return ST_E_ARG;
    VcfcMatrixArgs a;
    a.in = d_in; a.n_bytes = in_bytes; a.rec_start = d_rec; a.select = d_select; a.n = n; a.S = S; a.layout = layout;
    a.out = d_out; a.out_cap = out_cap; a.row_stride = row_stride; a.row_of = d_row_of;
    vcfc_matrix_args_workspace(a, static_cast<uint8_t *>(d_ws), L);
    a.err = d_err;
    return vcfc_matrix_run(a, s) == hipSuccess ? ST_OK : ST_E_HIP;
}

// records per batch where the caller names none: rows of at most 256 MiB
inline uint64_t default_batch(uint64_t row_bytes) {
    return std::max<uint64_t>(1, std::min<uint64_t>(1ull << 22, (256ull << 20) / row_bytes));
}

// The data section of a .vcfc (host bytes h_in[0, n); uploaded here).  q ==
// nullptr: every record gets a row; else the records the match step flags.
inline int matrix_section(const uint8_t *h_in, uint64_t n, uint64_t S, int layout, const vcfc_dec::MatchStep *q, Buffers &B,
                          hipStream_t s, Result &R, uint64_t rec_batch = 0) {
    R = Result();
    const uint64_t rb = vcfc_matrix_row_size(layout, S);
    if (!rb) return ST_E_ARG;
    if (!rec_batch) rec_batch = default_batch(rb);
    vcfc_dec::Section X;
    std::vector<uint8_t> flag;
    const int st = vcfc_dec::open_section(h_in, n, q, B, s, X, &flag);
    R.rec_start = X.rec;
    if (st) return st;
    const uint64_t nrec = X.nrec, k = X.k;   // records [0, k) are to be looked at
    std::vector<uint64_t> row_of;
    for (uint64_t i0 = 0; i0 < k; i0 += rec_batch) {
        const uint64_t nb = std::min(rec_batch, k - i0);
        const VcfcMatrixLayout L = vcfc_matrix_workspace_layout(nb);
        void *ws = B.get(Buffers::WS, L.total);
        uint8_t *d_rows = static_cast<uint8_t *>(B.get(Buffers::OUT, nb * rb + 64));
        uint64_t *d_row_of = static_cast<uint64_t *>(B.get(Buffers::LINE_OFF, 8 * (nb + 1)));
        if (!ws || !d_rows || !d_row_of) return ST_E_HIP;
        uint64_t err = 0;
        row_of.resize(nb + 1);
        if (matrix_device(X.d_in, n, X.d_rec + i0, X.d_flag ? X.d_flag + i0 : nullptr, nb, S, layout, d_rows, nb * rb, rb,
                          d_row_of, ws, L.total, X.d_small, s) != ST_OK ||
            hipMemcpyAsync(&err, X.d_small, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(row_of.data(), d_row_of, 8 * (nb + 1), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
        const uint64_t good = err == VCFCD_NO_ERROR ? nb : err >> 8;
        const uint64_t rows = row_of[good], have = R.rows.size();
        R.rows.resize(have + rows * rb);
        if (rows && (hipMemcpyAsync(R.rows.data() + have, d_rows, rows * rb, hipMemcpyDeviceToHost, s) != hipSuccess ||
                     hipStreamSynchronize(s) != hipSuccess))
            return ST_E_HIP;
        for (uint64_t j = 0; j < good; j++)
            if (!q || flag[i0 + j]) R.index.push_back(i0 + j);
        if (good < nb) {
            R.err_record = i0 + good;
            return ST_E_FORMAT;
        }
    }
    if (k < nrec || X.tail()) {
        R.err_record = k;
        return ST_E_FORMAT;
    }
    return ST_OK;
}

// A whole .vcfc: header, then matrix_section.
inline int matrix_file(const uint8_t *in, uint64_t n, int layout, const vcfc_dec::MatchStep *match, Buffers &B, hipStream_t s,
                       Result &R, uint64_t *data_off, uint64_t *S, uint64_t rec_batch = 0) {
    R = Result();
    if (!vcfc_matrix_row_size(layout, 1)) return ST_E_ARG;
    const int st = vcfc_cnt::counts_header(in, n, data_off, S);
    if (st) return st;
    return matrix_section(in + *data_off, n - *data_off, *S, layout, match, B, s, R, rec_batch);
}

// matrix_file with one region (q == nullptr: every record)
inline int matrix_file(const uint8_t *in, uint64_t n, int layout, const Query *q, Buffers &B, hipStream_t s, Result &R,
                       uint64_t *data_off, uint64_t *S, uint64_t rec_batch = 0) {
    R = Result();
    if (!q) return matrix_file(in, n, layout, static_cast<const vcfc_dec::MatchStep *>(nullptr), B, s, R, data_off, S, rec_batch);
    if (!vcfc_matrix_row_size(layout, 1)) return ST_E_ARG;
    VcfcQuery vq;
    const vcfc_dec::MatchStep match = vcfc_dec::region_step(q->ref, q->ref_len, q->has_range, q->start, q->end, &vq);
    const int st = vcfc_cnt::counts_header(in, n, data_off, S);
    if (st) return st;
    if (q->ref_len > 0xFFFFFFFFull) return ST_E_FORMAT;
    return matrix_section(in + *data_off, n - *data_off, *S, layout, &match, B, s, R, rec_batch);
}

// <prefix>.bed: PLINK 1's magic and variant-major mode byte, then the rows
inline void render_bed(const Result &R, std::vector<uint8_t> &out) {
    static const uint8_t magic[3] = {0x6C, 0x1B, 0x01};
    out.assign(magic, magic + 3);
    out.insert(out.end(), R.rows.begin(), R.rows.end());
}

// <prefix>.bim: per row CHROM ID 0 POS ALT REF, REQ's fields verbatim (data:
// the file's data section; a regular record has 9 TABs inside REQ)
inline void render_bim(const uint8_t *data, const Result &R, std::vector<uint8_t> &out) {
    out.clear();
    for (uint64_t r = 0; r < R.index.size(); r++) {
        const uint8_t *p = data + R.rec_start[R.index[r]] + 8;
        uint64_t f[6] = {0};   // starts of fields 0..4, and of field 5
        for (uint64_t e = 0, k = 1; k < 6; e++)
            if (p[e] == '\t') f[k++] = e + 1;
        auto put = [&](int k, char end) {
            out.insert(out.end(), p + f[k], p + f[k + 1] - 1);
            out.push_back((uint8_t)end);
        };
        put(0, '\t');
        put(2, '\t');
        out.push_back('0');
        out.push_back('\t');
        put(1, '\t');
        put(4, '\t');
        put(3, '\n');
    }
}

// <prefix>.fam: per sample its name from the '#CHROM' line, twice, and 0 0 0 -9
inline void render_fam(const uint8_t *in, uint64_t data_off, uint64_t S, std::vector<uint8_t> &out) {
    static const char rest[] = "\t0\t0\t0\t-9\n";
    out.clear();
    std::vector<uint64_t> f;
    vcfc_sub::header_fields(in, data_off, f);   // S + 9 fields
    for (uint64_t j = 0; j < S; j++) {
        out.insert(out.end(), in + f[9 + j], in + f[10 + j] - 1);
        out.push_back('\t');
        out.insert(out.end(), in + f[9 + j], in + f[10 + j] - 1);
        out.insert(out.end(), rest, rest + sizeof rest - 1);
    }
}

}  // namespace vcfc_gm
