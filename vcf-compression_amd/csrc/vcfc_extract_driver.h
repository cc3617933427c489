// vcfc_extract_driver.h -- host driver of extract, shared by
// the C ABI (vcfc_api.cpp) and the CPU emulator harness
// (tests/simt_emu/emu_extract_api.cpp), so the same control flow is tested on
// both.
//
//   1. the header, always: '##' lines verbatim, the '#CHROM' line cut as the
//      sample-subset decoder cuts it (verbatim with no column list);
//   2. hop the LEN headers on the host to find record starts; with a query,
//      flag the matching records (vcfc_dec::MatchStep: one region, or a
//      region table);
//   3. plan every taken record on the GPU exactly (record sizes, the first
//      one that is not regular or not re-encodable);
//   4. write the records before it in output batches, densely;
//   5. VCFC_E_FORMAT at that record, at a match error, or where hopping
//      stopped with 8 or more bytes left.
#pragma once
#include <cstdint>
#include <numeric>
#include <vector>

#include "vcfc_subset_driver.h"

namespace vcfc_ext {

using vcfc_dec::Buffers;
using vcfc_dec::Sink;
using vcfc_sub::ST_E_ARG;
using vcfc_sub::ST_E_FORMAT;
using vcfc_sub::ST_E_HIP;
using vcfc_sub::ST_E_IO;
using vcfc_sub::ST_OK;

// An upper bound on the bytes of an extract of n_records records, K columns,
// out of a file of in_bytes: the header is never longer than the input's; a
// record keeps its headers, REQ and LF, a chosen class token costs at most
// one run byte, and another chosen token its source bytes and terminator plus
// its own 0xE1 -- at most one byte a chosen column, and one for the source's
// last token, which has no terminator of its own.
inline uint64_t extract_bound(uint64_t in_bytes, uint64_t n_records, uint64_t K) { return in_bytes + n_records * (K + 1); }

// Header and sorted columns of an extract call.  cols == nullptr and K == 0:
// every column, in file order.
struct Call {
    std::vector<uint8_t> hdr;
    std::vector<uint32_t> all, csort, rank;
    uint64_t data_off = 0, S = 0;
    int prepare(const uint8_t *in, uint64_t n, const uint32_t *cols, uint64_t K) {
        int st = vcfc_dec::parse_header(in, n, &data_off, &S);
        if (st) return st;
        if (!cols && K == 0) {
            if (S == 0 || S >= (1ull << 31)) return ST_E_ARG;
            all.resize(S);
            std::iota(all.begin(), all.end(), 0u);
            hdr.assign(in, in + data_off);
            return vcfc_sub::sort_columns(all.data(), S, S, csort, rank);
        }
        st = vcfc_sub::subset_header(in, n, cols, K, hdr, &data_off, &S);
        if (!st) st = vcfc_sub::sort_columns(cols, K, S, csort, rank);
        return st;
    }
};

// The device entry's columns: the list, or 0 .. S - 1.
inline int device_columns(const uint32_t *cols, uint64_t K, uint64_t S, std::vector<uint32_t> &csort,
                          std::vector<uint32_t> &rank) {
    if (cols || K) return vcfc_sub::sort_columns(cols, K, S, csort, rank);
    if (S == 0 || S >= (1ull << 31)) return ST_E_ARG;
    std::vector<uint32_t> all(S);
    std::iota(all.begin(), all.end(), 0u);
    return vcfc_sub::sort_columns(all.data(), S, S, csort, rank);
}

// The output records of the records [rec[i], rec[i + 1]), i < nrec, of the
// uploaded data section (d_select, nullable: records with select[i] == 0 are
// not taken and not checked), sunk in order.  *stop = 1: a taken record is
// not regular or not re-encodable; the records before it are sunk.
inline int extract_records(const uint8_t *d_in, uint64_t n, uint64_t S, const uint64_t *d_rec, const uint8_t *d_select,
                           uint64_t nrec, const std::vector<uint32_t> &csort, const std::vector<uint32_t> &rank,
                           Buffers &B, hipStream_t s, const Sink &sink, uint64_t out_batch, int *stop) {
    *stop = 0;
    if (!nrec) return ST_OK;
    const uint64_t K = csort.size();
    const VcfcSubsetLayout L = vcfc_extract_workspace_layout(nrec, K);
    uint8_t *ws = static_cast<uint8_t *>(B.get(Buffers::WS, L.total));
    uint64_t *d_roff = static_cast<uint64_t *>(B.get(Buffers::LINE_OFF, 8 * (nrec + 1)));
    if (!ws || !d_roff) return ST_E_HIP;
    VcfcExtractArgs a;
    a.in = d_in; a.n_bytes = n; a.rec_start = d_rec; a.select = d_select; a.n = nrec; a.S = S; a.K = (uint32_t)K;
    a.out = nullptr; a.out_cap = 0; a.line_off = d_roff;
    vcfc_subset_args_workspace(a, ws, L);
    if (hipMemcpyAsync(ws + L.csort, csort.data(), 4 * K, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(ws + L.rank, rank.data(), 4 * K, hipMemcpyHostToDevice, s) != hipSuccess)
        return ST_E_HIP;
    uint64_t err = 0;
    if (vcfc_extract_plan(a, s) != hipSuccess || hipMemcpyAsync(&err, a.err, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return ST_E_HIP;
    uint64_t n_out = nrec;
    if (err != VCFCD_NO_ERROR) {
        n_out = err >> 8;
        *stop = 1;
    }
    std::vector<uint64_t> roff(n_out + 1);
    if (hipMemcpyAsync(roff.data(), d_roff, 8 * (n_out + 1), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return ST_E_HIP;
    for (uint64_t i0 = 0; i0 < n_out;) {
        uint64_t i1 = i0 + 1;
        while (i1 < n_out && roff[i1 + 1] - roff[i0] <= out_batch) i1++;
        const uint64_t bytes = roff[i1] - roff[i0];
        if (bytes) {
            uint8_t *d_out = static_cast<uint8_t *>(B.get(Buffers::OUT, bytes + 64));
            uint8_t *host = B.host(Buffers::HOST_OUT, bytes + 64);
            if (!d_out || !host) return ST_E_HIP;
            a.out = d_out - roff[i0];   // records are written at out + line_off[i]
            a.out_cap = roff[i1];
            if (vcfc_extract_write(a, i0, i1, s) != hipSuccess ||
                hipMemcpyAsync(host, d_out, bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess)
                return ST_E_HIP;
            if (!sink(host, bytes)) return ST_E_IO;
        }
        i0 = i1;
    }
    return ST_OK;
}

// The records (no header) of a .vcfc data section (host bytes h_in[0, n);
// uploaded here): all of them (match == nullptr), or those `match` flags;
// only taken records are checked.  A match error at record k stops there.
inline int extract_section(const uint8_t *h_in, uint64_t n, uint64_t S, const std::vector<uint32_t> &csort,
                           const std::vector<uint32_t> &rank, const vcfc_dec::MatchStep *match, Buffers &B, hipStream_t s,
                           const Sink &sink, uint64_t out_batch = 1ull << 30) {
    std::vector<uint64_t> rec;
    vcfc_dec::hop(h_in, n, rec);
    const uint64_t nrec = rec.size() - 1;
    if (nrec) {
        const uint8_t *d_in = vcfc_dec::upload(B, Buffers::IN, h_in, n, s);
        const uint64_t *d_rec = reinterpret_cast<const uint64_t *>(
            vcfc_dec::upload(B, Buffers::REC, reinterpret_cast<const uint8_t *>(rec.data()), 8 * rec.size(), s));
        if (!d_in || !d_rec) return ST_E_HIP;
        uint8_t *d_flag = nullptr;
        uint64_t k = nrec;   // the first record with a match error
        if (match) {
            const bool ready = match->prepare(B, s);
            uint64_t *d_small = static_cast<uint64_t *>(B.get(Buffers::SMALL, 64));
            d_flag = static_cast<uint8_t *>(B.get(Buffers::FLAG, nrec + 64));
            if (!ready || !d_small || !d_flag) return ST_E_HIP;
            uint64_t err = 0;
            if (match->run(d_in, d_rec, nrec, d_flag, d_small, s) != hipSuccess ||
                hipMemcpyAsync(&err, d_small, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess)
                return ST_E_HIP;
            if (err != VCFCD_NO_ERROR) k = err >> 8;
        }
        int stop = 0;
        const int st = extract_records(d_in, n, S, d_rec, d_flag, k, csort, rank, B, s, sink, out_batch, &stop);
        if (st) return st;
        if (stop || k < nrec) return ST_E_FORMAT;
    }
    return n - rec.back() >= 8 ? ST_E_FORMAT : ST_OK;   // fewer than 8 bytes left: a clean end
}

}  // namespace vcfc_ext
