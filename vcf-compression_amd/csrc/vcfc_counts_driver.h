// vcfc_counts_driver.h -- host driver of genotype-counts,
// shared by the C ABI (vcfc_api.cpp) and the CPU emulator harness
// (tests/simt_emu/emu_counts_api.cpp), so the same control flow is tested on
// both.
//
//   1. the header: S from the '#CHROM' line (ST_E_ARG for S == 0 or >= 2^30);
//   2. vcfc_dec::open_section: record starts, and with a query the flags of
//      the records to count, on the host too;
//   3. the records in batches of rec_batch: one scan each gives the batch's
//      rows and adds to the sample table, which stays on the device;
//   4. ST_E_FORMAT at the first counted record that is not regular, at a match
//      error, or where hopping stopped with 8 or more bytes left: the rows
//      before it are kept, the sample table is not.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vcfc_decode_driver.h"
#include "vcfc_device.h"
#include "vcfc_subset_driver.h"

namespace vcfc_cnt {

using vcfc_dec::Buffers;
constexpr int ST_OK = 0, ST_E_ARG = 5, ST_E_HIP = 6, ST_E_IO = 7, ST_E_FORMAT = 8;   // = include/vcfc.h codes

struct Query {
    const uint8_t *ref;
    uint64_t ref_len;
    int has_range;
    uint64_t start, end;
};

struct Result {
    std::vector<uint64_t> index;     // file index of each counted record
    std::vector<uint32_t> rows;      // 8 per counted record
    std::vector<uint64_t> samples;   // 5 S (ST_OK only)
    uint64_t err_record = ~0ull;     // the record the call stopped at
    std::vector<uint64_t> rec_start; // the hopped records' offsets in the data section
};

// S of a header parse_header accepts: ST_E_ARG outside [1, 2^30)
inline int counts_header(const uint8_t *in, uint64_t n, uint64_t *data_off, uint64_t *S) {
    const int st = vcfc_dec::parse_header(in, n, data_off, S);
    if (st) return st;
    return *S == 0 || *S >= (1ull << 30) ? ST_E_ARG : ST_OK;
}

// The device entry (include/vcfc.h: vcfc_genotype_counts_device): argument
// checks, then the kernels enqueued on s.
inline int counts_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec, const uint8_t *d_select, uint64_t n,
                         uint64_t S, uint32_t *d_variant, uint64_t *d_sample, void *d_ws, uint64_t ws_bytes,
                         uint64_t *d_err, hipStream_t s) {
    if ((n && (!d_in || !d_rec)) || (!d_variant && !d_sample) || !d_ws || !d_err) return ST_E_ARG;
    // S < 2^30 keeps every 32-bit counter exact (vcfc_counts.hip); n < 2^32: the queue holds 32-bit indices
    if (S == 0 || S >= (1ull << 30) || n >= (1ull << 32)) return ST_E_ARG;
    const VcfcCountsLayout L = vcfc_counts_workspace_layout(n, S);
    if (ws_bytes < L.total) return ST_E_ARG;
    VcfcCountsArgs a;
    a.in = d_in; a.n_bytes = in_bytes; a.rec_start = d_rec; a.select = d_select; a.n = n; a.S = S;
    a.variant = d_variant; a.sample = d_sample;
    vcfc_counts_args_workspace(a, static_cast<uint8_t *>(d_ws), L);
    a.err = d_err;
    return vcfc_counts_run(a, s) == hipSuccess ? ST_OK : ST_E_HIP;
}

// The data section of a .vcfc (host bytes h_in[0, n); uploaded here).  q ==
// nullptr: every record is counted; else the records the match step flags
// (vcfc_dec::MatchStep: one region, or a region table).
inline int counts_section(const uint8_t *h_in, uint64_t n, uint64_t S, const vcfc_dec::MatchStep *q, Buffers &B,
                          hipStream_t s, Result &R, uint64_t rec_batch = 1ull << 22) {
    R = Result();
    // the sample table is zeroed ahead of the match step, on a file with no record too
    uint64_t *d_sample = static_cast<uint64_t *>(B.get(Buffers::LINE_OFF, 40 * S));
    if (!d_sample || hipMemsetAsync(d_sample, 0, 40 * S, s) != hipSuccess) return ST_E_HIP;
    vcfc_dec::Section X;
    std::vector<uint8_t> flag;
    const int st = vcfc_dec::open_section(h_in, n, q, B, s, X, &flag);
    R.rec_start = X.rec;
    if (st) return st;
    const uint64_t nrec = X.nrec, k = X.k;   // records [0, k) are to be counted
    for (uint64_t i0 = 0; i0 < k; i0 += rec_batch) {
        const uint64_t nb = std::min(rec_batch, k - i0);
        const VcfcCountsLayout L = vcfc_counts_workspace_layout(nb, S);
        uint8_t *ws = static_cast<uint8_t *>(B.get(Buffers::WS, L.total));
        uint32_t *d_rows = static_cast<uint32_t *>(B.get(Buffers::OUT, 32 * nb + 64));
        if (!ws || !d_rows) return ST_E_HIP;
        VcfcCountsArgs a;
        a.in = X.d_in; a.n_bytes = n; a.rec_start = X.d_rec + i0; a.select = X.d_flag ? X.d_flag + i0 : nullptr; a.n = nb;
        a.S = S; a.variant = d_rows; a.sample = d_sample;
        vcfc_counts_args_workspace(a, ws, L);
        uint64_t err = 0;
        if (vcfc_counts_run(a, s) != hipSuccess || hipMemcpyAsync(&err, a.err, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
        const uint64_t good = err == VCFCD_NO_ERROR ? nb : err >> 8;
        std::vector<uint32_t> rows(8 * good);
        if (good && (hipMemcpyAsync(rows.data(), d_rows, 32 * good, hipMemcpyDeviceToHost, s) != hipSuccess ||
                     hipStreamSynchronize(s) != hipSuccess))
            return ST_E_HIP;
        for (uint64_t j = 0; j < good; j++) {
            if (q && !flag[i0 + j]) continue;
            R.index.push_back(i0 + j);
            R.rows.insert(R.rows.end(), rows.begin() + 8 * j, rows.begin() + 8 * j + 8);
        }
        if (good < nb) {
            R.err_record = i0 + good;
            return ST_E_FORMAT;
        }
    }
    if (k < nrec || X.tail()) {
        R.err_record = k;
        return ST_E_FORMAT;
    }
    R.samples.resize(5 * S);
    if (hipMemcpyAsync(R.samples.data(), d_sample, 40 * S, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return ST_E_HIP;
    return ST_OK;
}

// A whole .vcfc: header, then counts_section.
inline int counts_file(const uint8_t *in, uint64_t n, const vcfc_dec::MatchStep *match, Buffers &B, hipStream_t s, Result &R,
                       uint64_t *data_off, uint64_t *S, uint64_t rec_batch = 1ull << 22) {
    R = Result();
    const int st = counts_header(in, n, data_off, S);
    if (st) return st;
    return counts_section(in + *data_off, n - *data_off, *S, match, B, s, R, rec_batch);
}

// counts_file with one region (q == nullptr: every record)
inline int counts_file(const uint8_t *in, uint64_t n, const Query *q, Buffers &B, hipStream_t s, Result &R,
                       uint64_t *data_off, uint64_t *S, uint64_t rec_batch = 1ull << 22) {
    R = Result();
    if (!q) return counts_file(in, n, static_cast<const vcfc_dec::MatchStep *>(nullptr), B, s, R, data_off, S, rec_batch);
    VcfcQuery vq;
    const vcfc_dec::MatchStep match = vcfc_dec::region_step(q->ref, q->ref_len, q->has_range, q->start, q->end, &vq);
    const int st = counts_header(in, n, data_off, S);
    if (st) return st;
    if (q->ref_len > 0xFFFFFFFFull) return ST_E_FORMAT;
    return counts_section(in + *data_off, n - *data_off, *S, &match, B, s, R, rec_batch);
}

inline void put_numbers(std::vector<uint8_t> &out, const uint64_t *v, int k) {
    char buf[24];
    for (int j = 0; j < k; j++) {
        const int len = snprintf(buf, sizeof buf, "\t%llu", (unsigned long long)v[j]);
        out.insert(out.end(), buf, buf + len);
    }
    out.push_back('\n');
}

// variants.tsv: the header line, then per counted record REQ's first two
// fields verbatim and the eight numbers (data: the file's data section)
inline void render_variants(const uint8_t *data, const Result &R, std::vector<uint8_t> &out) {
    static const char head[] = "#CHROM\tPOS\tN_00\tN_01\tN_10\tN_11\tN_OTHER\tAN\tAC1\tAC_OTHER\n";
    out.assign(head, head + sizeof head - 1);
    for (uint64_t r = 0; r < R.index.size(); r++) {
        const uint8_t *p = data + R.rec_start[R.index[r]] + 8;   // a regular record: 9 TABs inside REQ
        uint64_t e = 0;
        for (int tabs = 0;; e++)
            if (p[e] == '\t' && ++tabs == 2) break;
        out.insert(out.end(), p, p + e);
        uint64_t v[8];
        for (int j = 0; j < 8; j++) v[j] = R.rows[8 * r + j];
        put_numbers(out, v, 8);
    }
}

// samples.tsv: the header line, then per sample its name verbatim from the
// '#CHROM' line and the five numbers
inline void render_samples(const uint8_t *in, uint64_t data_off, uint64_t S, const Result &R, std::vector<uint8_t> &out) {
    static const char head[] = "#SAMPLE\tN_00\tN_01\tN_10\tN_11\tN_OTHER\n";
    out.assign(head, head + sizeof head - 1);
    std::vector<uint64_t> f;
    vcfc_sub::header_fields(in, data_off, f);   // S + 9 fields
    for (uint64_t j = 0; j < S; j++) {
        out.insert(out.end(), in + f[9 + j], in + f[10 + j] - 1);
        put_numbers(out, R.samples.data() + 5 * j, 5);
    }
}

}  // namespace vcfc_cnt
