// vcfc_subset_driver.h -- host driver of the sample-subset decoder
// (DESIGN.md §4i), shared by the C ABI (vcfc_api.cpp) and the CPU emulator
// harness (tests/simt_emu/emu_subset_api.cpp), so the same control flow is
// tested on both.
//
//   1. the header: '##' lines verbatim, the '#CHROM' line cut to its first 9
//      fields and the chosen names;
//   2. vcfc_dec::open_section: record starts, and with a query the flags of
//      the matching records (vcfc_dec::MatchStep: the range query's, kernel
//      and error word unchanged, or a region table's);
//   3. plan every taken record on the GPU exactly (line sizes, first
//      irregular one);
//   4. write the lines before it in output batches;
//   5. VCFC_E_FORMAT at that record, at a match error, or where hopping
//      stopped with 8 or more bytes left.
// Extract (vcfc_extract_driver.h) runs steps 2 to 5 with its own kernels.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "vcfc_decode_driver.h"
#include "vcfc_device.h"

namespace vcfc_sub {

using vcfc_dec::Buffers;
using vcfc_dec::Sink;
constexpr int ST_OK = 0, ST_E_ARG = 5, ST_E_HIP = 6, ST_E_IO = 7, ST_E_FORMAT = 8;   // = include/vcfc.h codes

// The chosen columns, ascending, and each one's output slot.  ST_E_ARG: no
// column, a column >= S, a column listed twice.
inline int sort_columns(const uint32_t *cols, uint64_t K, uint64_t S, std::vector<uint32_t> &csort,
                        std::vector<uint32_t> &rank) {
    if (!cols || K == 0 || K > S || S >= (1ull << 31)) return ST_E_ARG;
    rank.resize(K);
    std::iota(rank.begin(), rank.end(), 0u);
    std::sort(rank.begin(), rank.end(), [&](uint32_t x, uint32_t y) { return cols[x] < cols[y]; });
    csort.resize(K);
    for (uint64_t k = 0; k < K; k++) csort[k] = cols[rank[k]];
    if (csort[K - 1] >= S) return ST_E_ARG;
    for (uint64_t k = 1; k < K; k++)
        if (csort[k] == csort[k - 1]) return ST_E_ARG;
    return ST_OK;
}

// sort_columns of the list, or, where the caller allows it (extract), of
// 0 .. S - 1 for cols == nullptr and K == 0.
inline int choose_columns(const uint32_t *cols, uint64_t K, uint64_t S, bool all_ok, std::vector<uint32_t> &csort,
                          std::vector<uint32_t> &rank) {
    if (cols || K || !all_ok) return sort_columns(cols, K, S, csort, rank);
    if (S == 0 || S >= (1ull << 31)) return ST_E_ARG;
    std::vector<uint32_t> all(S);
    std::iota(all.begin(), all.end(), 0u);
    return sort_columns(all.data(), S, S, csort, rank);
}

// The fields of the '#CHROM' line of a header parse_header accepts:
// f[j] = offset of field j, f.back() = the line's LF + 1 (= data_off).
inline void header_fields(const uint8_t *in, uint64_t data_off, std::vector<uint64_t> &f) {
    uint64_t ls = data_off - 1;   // the line's LF
    while (ls > 0 && in[ls - 1] != '\n') ls--;
    f.clear();
    f.push_back(ls);
    for (uint64_t k = ls; k + 1 < data_off; k++)
        if (in[k] == '\t') f.push_back(k + 1);
    f.push_back(data_off);
}

// The subset's header.  ST_E_FORMAT where parse_header fails, ST_E_ARG for a
// column >= S (sort_columns checks the rest).
inline int subset_header(const uint8_t *in, uint64_t n, const uint32_t *cols, uint64_t K, std::vector<uint8_t> &hdr,
                         uint64_t *data_off, uint64_t *S) {
    int st = vcfc_dec::parse_header(in, n, data_off, S);
    if (st) return st;
    if (!cols || K == 0) return ST_E_ARG;
    for (uint64_t k = 0; k < K; k++)
        if (cols[k] >= *S) return ST_E_ARG;
    std::vector<uint64_t> f;
    header_fields(in, *data_off, f);   // S + 9 fields
    hdr.assign(in, in + f[9] - 1);     // through the 9th field, without its TAB
    for (uint64_t k = 0; k < K; k++) {
        hdr.push_back('\t');
        hdr.insert(hdr.end(), in + f[9 + cols[k]], in + f[10 + cols[k]] - 1);
    }
    hdr.push_back('\n');
    return ST_OK;
}

// Header and sorted columns of a whole-file call.  all_ok (extract): cols ==
// nullptr and K == 0 keep the header verbatim and every column.
struct Call {
    std::vector<uint8_t> hdr;
    std::vector<uint32_t> csort, rank;
    uint64_t data_off = 0, S = 0;
    int prepare(const uint8_t *in, uint64_t n, const uint32_t *cols, uint64_t K, bool all_ok = false) {
        if (all_ok && !cols && K == 0) {
            const int st = vcfc_dec::parse_header(in, n, &data_off, &S);
            if (st) return st;
            hdr.assign(in, in + data_off);
        } else {
            const int st = subset_header(in, n, cols, K, hdr, &data_off, &S);
            if (st) return st;
        }
        return choose_columns(cols, K, S, all_ok, csort, rank);
    }
};

// The three entry points in which the sample-subset decoder and extract
// differ (vcfc_device.h); both use VcfcSubsetArgs and VcfcSubsetLayout.
struct Kernels {
    VcfcSubsetLayout (*layout)(uint64_t n, uint64_t K);
    hipError_t (*plan)(const VcfcSubsetArgs &a, hipStream_t s);
    hipError_t (*write)(const VcfcSubsetArgs &a, uint64_t first, uint64_t last, hipStream_t s);
};
constexpr Kernels SUBSET = {vcfc_subset_workspace_layout, vcfc_subset_plan, vcfc_subset_write};

// The body of the two device entries (include/vcfc.h: vcfc_decode_samples_device,
// vcfc_extract_samples_device) behind their pointer and column checks: the
// workspace check, then plan and write enqueued on s.
inline int records_device(const Kernels &kn, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec,
                          const uint8_t *d_select, uint64_t n, uint64_t S, const std::vector<uint32_t> &csort,
                          const std::vector<uint32_t> &rank, uint8_t *d_out, uint64_t out_cap, uint64_t *d_off, void *d_ws,
                          uint64_t ws_bytes, uint64_t *d_err, hipStream_t s) {
    const uint64_t K = csort.size();
    const VcfcSubsetLayout L = kn.layout(n, K);
    if (ws_bytes < L.total) return 4;   // VCFC_E_NOSPACE
    uint8_t *ws = static_cast<uint8_t *>(d_ws);
    VcfcSubsetArgs a;
    a.in = d_in; a.n_bytes = in_bytes; a.rec_start = d_rec; a.select = d_select; a.n = n; a.S = S; a.K = (uint32_t)K;
    a.out = d_out; a.out_cap = out_cap; a.line_off = d_off;
    vcfc_subset_args_workspace(a, ws, L);
    a.err = d_err;
    // csort and rank live on the caller's frame: the stream has taken them when the synchronise returns
    if (hipMemcpyAsync(ws + L.csort, csort.data(), 4 * K, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(ws + L.rank, rank.data(), 4 * K, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return ST_E_HIP;
    if (kn.plan(a, s) != hipSuccess) return ST_E_HIP;
    return kn.write(a, 0, n, s) == hipSuccess ? ST_OK : ST_E_HIP;
}

// The output (kn: lines, or extract's records) of the records [rec[i],
// rec[i + 1]), i < nrec, of the uploaded data section (d_select, nullable:
// records with select[i] == 0 give nothing and are not checked), sunk in
// order.  *stop = 1: a record is not regular (extract: or not re-encodable);
// the output before it is sunk.
inline int subset_records(const Kernels &kn, const uint8_t *d_in, uint64_t n, uint64_t S, const uint64_t *d_rec,
                          const uint8_t *d_select, uint64_t nrec, const std::vector<uint32_t> &csort,
                          const std::vector<uint32_t> &rank, Buffers &B, hipStream_t s, const Sink &sink, uint64_t out_batch,
                          int *stop) {
    *stop = 0;
    if (!nrec) return ST_OK;
    const uint64_t K = csort.size();
    const VcfcSubsetLayout L = kn.layout(nrec, K);
    uint8_t *ws = static_cast<uint8_t *>(B.get(Buffers::WS, L.total));
    uint64_t *d_loff = static_cast<uint64_t *>(B.get(Buffers::LINE_OFF, 8 * (nrec + 1)));
    if (!ws || !d_loff) return ST_E_HIP;
    VcfcSubsetArgs a;
    a.in = d_in; a.n_bytes = n; a.rec_start = d_rec; a.select = d_select; a.n = nrec; a.S = S; a.K = (uint32_t)K;
    a.out = nullptr; a.out_cap = 0; a.line_off = d_loff;
    vcfc_subset_args_workspace(a, ws, L);
    if (hipMemcpyAsync(ws + L.csort, csort.data(), 4 * K, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(ws + L.rank, rank.data(), 4 * K, hipMemcpyHostToDevice, s) != hipSuccess)
        return ST_E_HIP;
    uint64_t err = 0;
    if (kn.plan(a, s) != hipSuccess || hipMemcpyAsync(&err, a.err, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return ST_E_HIP;
    uint64_t n_lines = nrec;
    if (err != VCFCD_NO_ERROR) {
        n_lines = err >> 8;
        *stop = 1;
    }
    std::vector<uint64_t> loff(n_lines + 1);
    if (hipMemcpyAsync(loff.data(), d_loff, 8 * (n_lines + 1), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return ST_E_HIP;
    for (uint64_t i0 = 0; i0 < n_lines;) {
        uint64_t i1 = i0 + 1;
        while (i1 < n_lines && loff[i1 + 1] - loff[i0] <= out_batch) i1++;
        const uint64_t bytes = loff[i1] - loff[i0];
        if (bytes) {
            uint8_t *d_out = static_cast<uint8_t *>(B.get(Buffers::OUT, bytes + 64));
            uint8_t *host = B.host(Buffers::HOST_OUT, bytes + 64);
            if (!d_out || !host) return ST_E_HIP;
            a.out = d_out - loff[i0];   // lines are written at out + line_off[i]
            a.out_cap = loff[i1];
            if (kn.write(a, i0, i1, s) != hipSuccess ||
                hipMemcpyAsync(host, d_out, bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess)
                return ST_E_HIP;
            if (!sink(host, bytes)) return ST_E_IO;
        }
        i0 = i1;
    }
    return ST_OK;
}

// The output (no header) of a .vcfc data section (host bytes h_in[0, n);
// uploaded by vcfc_dec::open_section): of every record (match == nullptr), or
// of those `match` flags (one region, or a region table); only taken records
// must be regular.  ST_E_FORMAT at the first one that is not, at a match error
// at record k (the output of the records before it sunk), or where hopping
// stopped with 8 or more bytes left.
inline int subset_section(const Kernels &kn, const uint8_t *h_in, uint64_t n, uint64_t S, const std::vector<uint32_t> &csort,
                          const std::vector<uint32_t> &rank, const vcfc_dec::MatchStep *match, Buffers &B, hipStream_t s,
                          const Sink &sink, uint64_t out_batch = 1ull << 30) {
    vcfc_dec::Section X;
    int st = vcfc_dec::open_section(h_in, n, match, B, s, X);
    if (st) return st;
    int stop = 0;
    st = subset_records(kn, X.d_in, n, S, X.d_rec, X.d_flag, X.k, csort, rank, B, s, sink, out_batch, &stop);
    if (st) return st;
    return stop || X.k < X.nrec || X.tail() ? ST_E_FORMAT : ST_OK;
}

// The subset decoder's two names for subset_section with its own kernels, as
// vcfc_ext::extract_section is extract's: every record's lines, and the lines
// of the records `match` flags.
inline int decode_section(const uint8_t *h_in, uint64_t n, uint64_t S, const std::vector<uint32_t> &csort,
                          const std::vector<uint32_t> &rank, Buffers &B, hipStream_t s, const Sink &sink,
                          uint64_t out_batch = 1ull << 30) {
    return subset_section(SUBSET, h_in, n, S, csort, rank, nullptr, B, s, sink, out_batch);
}
inline int matched_section(const uint8_t *h_in, uint64_t n, uint64_t S, const std::vector<uint32_t> &csort,
                           const std::vector<uint32_t> &rank, const vcfc_dec::MatchStep &match, Buffers &B, hipStream_t s,
                           const Sink &sink, uint64_t out_batch = 1ull << 30) {
    return subset_section(SUBSET, h_in, n, S, csort, rank, &match, B, s, sink, out_batch);
}

// matched_section with one region: matched exactly as vcfc_dec::query_section
// matches.
inline int query_section(const uint8_t *h_in, uint64_t n, uint64_t S, const std::vector<uint32_t> &csort,
                         const std::vector<uint32_t> &rank, const uint8_t *qref, uint64_t qref_len, int has_range,
                         uint64_t qstart, uint64_t qend, Buffers &B, hipStream_t s, const Sink &sink,
                         uint64_t out_batch = 1ull << 30) {
    if (qref_len > 0xFFFFFFFFull) return ST_E_FORMAT;
    VcfcQuery q;
    return matched_section(h_in, n, S, csort, rank, vcfc_dec::region_step(qref, qref_len, has_range, qstart, qend, &q), B, s,
                           sink, out_batch);
}

// Resolve a comma-separated name list against the '#CHROM' line (the first
// occurrence wins where the header repeats a name).  ST_E_ARG with *bad_off =
// the offset in `names` of a name the header lacks, or of a name's second
// listing; 4 (VCFC_E_NOSPACE) with *n_cols set where cols_cap is short.
inline int sample_columns(const uint8_t *in, uint64_t n, const char *names, uint64_t names_len, uint32_t *cols,
                          uint64_t cols_cap, uint64_t *n_cols, uint64_t *bad_off) {
    uint64_t data_off = 0, S = 0;
    const int st = vcfc_dec::parse_header(in, n, &data_off, &S);
    if (st) return st;
    std::vector<uint64_t> f;
    header_fields(in, data_off, f);
    std::vector<uint32_t> got;
    for (uint64_t a = 0;;) {
        uint64_t b = a;
        while (b < names_len && names[b] != ',') b++;
        uint64_t col = S;
        for (uint64_t j = 0; j < S && col == S; j++) {
            const uint64_t f0 = f[9 + j], f1 = f[10 + j] - 1;
            if (f1 - f0 == b - a && memcmp(in + f0, names + a, b - a) == 0) col = j;
        }
        if (col == S || std::find(got.begin(), got.end(), (uint32_t)col) != got.end()) {
            *bad_off = a;
            return ST_E_ARG;
        }
        got.push_back((uint32_t)col);
        if (b >= names_len) break;
        a = b + 1;
    }
    *n_cols = got.size();
    if (got.size() > cols_cap) return 4;
    std::copy(got.begin(), got.end(), cols);
    return ST_OK;
}

}  // namespace vcfc_sub
