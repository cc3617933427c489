// vcfc_sparse_index_driver.h -- host drivers of the sparse external index,
// shared by the C ABI (vcfc_api.cpp) and the CPU emulator harness
// (tests/simt_emu/emu_sparse_index_api.cpp), so the same control flow is
// tested on both.
//
// create (create_sparse_external_index, reference src/main.cpp:854-999):
//   1. parse the header, hop the LEN headers on the host;
//   2. upload the data section; vcfc_sparse_index_build computes every
//      record's ref_idx and POS, the slot offsets, which record of each slot
//      is the last writer, and the kept entries, densely;
//   3. the reference writes one entry per record, in order, and stops at the
//      first record it throws on or cannot seek to.  Without such a record
//      and with offsets that never decrease, only the kept entries are
//      written, those of one 4 KiB block in one pwrite.  Otherwise the
//      records before the stopping one are written one by one in order.
// query (query_sparse_external_index, :1002-1281):
//   1. the reference's slot lookup on the index: the entry at the slot of
//      `start`, else (for start != end) the first non-zero slot after it,
//      holes skipped with SEEK_DATA;
//   2. from the entry's byte_offset the file is read in windows; per window:
//      hop, the walk span (CHROM and POS only), k_index_compare with end =
//      pos (compare_to, :88-108), decode_records with the flags;
//   3. stop at the window holding the first record after the query, or EOF.
// gap-analysis (gap_analysis, :3931-3980): the exact decode plan without the
// write pass, a per-record field pass, and text formatting on the host.
#pragma once
#include <cstdio>

#include "vcfc_index_driver.h"

namespace vcfc_spx {

using vcfc_dec::Buffers;
using vcfc_dec::Sink;
using vcfc_idx::ENTRY_BYTES;
using vcfc_idx::Reader;
using vcfc_idx::ST_E_FORMAT;
using vcfc_idx::ST_E_HIP;
using vcfc_idx::ST_E_IO;
using vcfc_idx::ST_OK;
constexpr uint64_t SLOT_BYTES = 256;       // SPARSE_EXTERNAL_INDEX_BLOCK_SIZE x multiplication_factor 1 (:4152-4155)
constexpr uint64_t MAX_POSITION = 300000000;   // SparsificationConfiguration::max_position (src/sparse.hpp:29-32)
constexpr uint64_t WRITE_BLOCK = 4096;
constexpr uint64_t SEEK_DATA_PROBE = 10000000;   // test_seek_data_offset (:1041)

// compute_sparse_offset (src/sparse.cpp:18-51), 64-bit wrap-around
inline uint64_t slot_offset(uint64_t pos) { return (MAX_POSITION + pos) * SLOT_BYTES; }

// the index being written.  0: written; 1: the file system refuses the
// offset (EINVAL / EFBIG: the reference's lseek fails there); -1: I/O error
struct Writer {
    virtual ~Writer() {}
    virtual int pwrite(const uint8_t *p, uint64_t k, uint64_t off) = 0;
};

struct CreateStats {
    uint64_t records = 0, entries = 0, pwrites = 0;
    int in_order = 0;   // 1: the record-by-record path was taken
};

inline void pack_entry(uint8_t *e, uint32_t ref, uint64_t pos, uint64_t off) {
    e[0] = (uint8_t)ref;
    for (int k = 0; k < 4; k++) e[1 + k] = (uint8_t)(pos >> (8 * k));
    for (int k = 0; k < 8; k++) e[5 + k] = (uint8_t)(off >> (8 * k));
}

// The index of a whole .vcfc (host bytes) into W.  *err_record: the first
// record the reference throws on (ST_E_FORMAT), else -1; *seek_failed = 1
// where the reference's lseek to a slot fails (ST_OK, :954-959).  Either way
// the entries of the records before it are written.
inline int create_index(const uint8_t *h_in, uint64_t n_bytes, Buffers &B, hipStream_t s, Writer &W,
                        int64_t *err_record, int *seek_failed, CreateStats *stats = nullptr) {
    if (err_record) *err_record = -1;
    if (seek_failed) *seek_failed = 0;
    uint64_t data_off = 0;
    int st = vcfc_dec::parse_header(h_in, n_bytes, &data_off, nullptr);
    if (st) return st;
    const uint8_t *data = h_in + data_off;
    std::vector<uint64_t> rec;
    const int why = vcfc_idx::hop_why(data, n_bytes - data_off, rec);
    const uint64_t nrec = rec.size() - 1;
    if (stats) stats->records = nrec;
    uint64_t words[5] = {VCFCD_NO_ERROR, 0, 0, 0, ~0ull};   // err, count, status[0..2]
    const VcfcSparseIndexLayout L = vcfc_sparse_index_workspace_layout(nrec);
    uint8_t *ws = nullptr, *d_entries = nullptr;
    uint64_t *d_off = nullptr;
    if (nrec) {
        const uint8_t *d_in = vcfc_dec::upload(B, Buffers::IN, data, rec[nrec], s);
        const uint64_t *d_rec = reinterpret_cast<const uint64_t *>(
            vcfc_dec::upload(B, Buffers::REC, reinterpret_cast<const uint8_t *>(rec.data()), 8 * (nrec + 1), s));
        ws = static_cast<uint8_t *>(B.get(Buffers::WS, L.total));
        d_entries = static_cast<uint8_t *>(B.get(Buffers::OUT, ENTRY_BYTES * nrec + 64));
        d_off = static_cast<uint64_t *>(B.get(Buffers::LINE_OFF, 8 * nrec + 64));
        uint64_t *d_small = static_cast<uint64_t *>(B.get(Buffers::SMALL, 64));
        if (!d_in || !d_rec || !ws || !d_entries || !d_off || !d_small) return ST_E_HIP;
        if (vcfc_sparse_index_build(d_in, d_rec, nrec, data_off, d_entries, d_off, d_small + 1, d_small + 2, ws, L,
                                    d_small, s) != hipSuccess ||
            hipMemcpyAsync(words, d_small, 40, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
    }
    // the first stopping record: a throw comes before the seek of the same record
    const uint64_t bad = words[0] == VCFCD_NO_ERROR ? ~0ull : words[0] >> 8;
    const uint64_t hdr = why != vcfc_idx::HOP_END ? nrec : ~0ull;   // a record header the reference cannot read
    const uint64_t seek = words[4];
    const uint64_t stop = std::min(std::min(bad, hdr), seek);
    const bool thrown = stop != ~0ull && (bad == stop || hdr == stop);
    const uint64_t upto = std::min(stop, nrec);
    if (upto && (stop != ~0ull || words[3])) {
        // record by record, in order: the later writer of a slot wins
        std::vector<uint8_t> ref(upto);
        std::vector<uint64_t> pos(upto);
        if (hipMemcpyAsync(ref.data(), ws + L.ref_idx, upto, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(pos.data(), ws + L.pos, 8 * upto, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
        if (stats) { stats->in_order = 1; stats->entries = upto; stats->pwrites = upto; }
        uint8_t e[ENTRY_BYTES];
        for (uint64_t i = 0; i < upto; i++) {
            pack_entry(e, ref[i], pos[i], data_off + rec[i]);
            const int rc = W.pwrite(e, ENTRY_BYTES, slot_offset(pos[i]));
            if (rc < 0) return ST_E_IO;
            if (rc > 0) {   // later records are never looked at (:954-959)
                if (seek_failed) *seek_failed = 1;
                return ST_OK;
            }
        }
    } else if (upto) {
        const uint64_t cnt = words[1];
        std::vector<uint8_t> ent(ENTRY_BYTES * cnt);
        std::vector<uint64_t> off(cnt);
        if (hipMemcpyAsync(ent.data(), d_entries, ent.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(off.data(), d_off, 8 * cnt, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
        if (stats) stats->entries = cnt;
        // offsets increase strictly here; the entries of one 4 KiB block go
        // out as one write of the span between them (the file was truncated:
        // the bytes between entries are zeros either way)
        uint8_t blk[WRITE_BLOCK];
        for (uint64_t j = 0; j < cnt;) {
            const uint64_t o0 = off[j], lim = (o0 / WRITE_BLOCK + 1) * WRITE_BLOCK;
            uint64_t k = j, len = 0;
            memset(blk, 0, sizeof(blk));
            for (; k < cnt && off[k] + ENTRY_BYTES <= lim && off[k] >= o0; k++) {
                memcpy(blk + (off[k] - o0), ent.data() + ENTRY_BYTES * k, ENTRY_BYTES);
                len = off[k] - o0 + ENTRY_BYTES;
            }
            const int rc = W.pwrite(blk, len, o0);
            if (rc < 0) return ST_E_IO;
            if (rc > 0) {   // offsets only grow from here: the first refused record stops the run
                if (seek_failed) *seek_failed = 1;
                return ST_OK;
            }
            if (stats) stats->pwrites++;
            j = k;
        }
    }
    if (thrown) {
        if (err_record) *err_record = (int64_t)stop;
        return ST_E_FORMAT;
    }
    if (stop != ~0ull && seek_failed) *seek_failed = 1;
    return ST_OK;
}

// the index being queried: bytes [off, off + k) (short only at EOF, -1 on an
// error), and lseek(off, SEEK_DATA): the first offset >= off that holds data,
// -1 where there is none
struct IndexFile {
    virtual ~IndexFile() {}
    virtual int64_t pread(uint8_t *dst, uint64_t off, uint64_t k) = 0;
    virtual int64_t seek_data(uint64_t off) = 0;
};

// The lookup of :1069-1174.  0: *out is the entry; 1: no output.
inline int lookup(IndexFile &I, uint64_t qstart, uint64_t qend, vcfc_idx::Entry *out) {
    auto zero = [](const vcfc_idx::Entry &e) { return e.ref == 0 && e.pos == 0 && e.off == 0; };
    uint64_t cur = slot_offset(qstart);
    if ((int64_t)cur < 0) return 1;   // lseek: Invalid argument
    uint8_t b[ENTRY_BYTES];
    if (I.pread(b, cur, ENTRY_BYTES) != (int64_t)ENTRY_BYTES) return 1;   // at or past EOF
    vcfc_idx::Entry e = vcfc_idx::get_entry(b, 0);
    if (zero(e)) {
        if (qstart == qend) return 1;   // the queried variant does not exist
        while (true) {
            const int64_t d = I.seek_data(cur);
            if (d < 0) return 1;
            cur = (uint64_t)d;
            if (I.pread(b, cur, ENTRY_BYTES) != (int64_t)ENTRY_BYTES) return 1;
            e = vcfc_idx::get_entry(b, 0);
            if (!zero(e)) break;
            cur += SLOT_BYTES;
        }
    }
    *out = e;
    return 0;
}

// Indexed query: the lines of the records from the looked-up entry on that
// compare_to places in (ref, start, end), up to the first record after it.
// Records before the query are skipped without being decoded.  No byte of
// the .vcfc before that entry's byte_offset is read, apart from the header.
inline int query_index(Reader &R, IndexFile &I, const uint8_t *qref, uint64_t qref_len, int has_range,
                       uint64_t qstart, uint64_t qend, Buffers &B, hipStream_t s, const Sink &sink,
                       uint64_t window_bytes = 4ull << 20, vcfc_idx::QueryStats *stats = nullptr,
                       uint64_t out_batch = 1ull << 30) {
    const uint64_t fsize = R.size();
    // the SEEK_DATA probe of :1040-1047 comes before the header is read: an
    // index without an entry gives no output, whatever the .vcfc holds
    if (I.seek_data(SEEK_DATA_PROBE) < 0) return ST_OK;
    // decompress2_metadata_headers over a growing prefix
    uint64_t data_off = 0, S = 0;
    {
        std::vector<uint8_t> hb;
        for (uint64_t hn = 1ull << 16;; hn *= 4) {
            hb.resize(std::min(hn, fsize));
            const int64_t got = R.read(hb.data(), 0, hb.size());
            if (got < 0) return ST_E_IO;
            if (vcfc_dec::parse_header(hb.data(), (uint64_t)got, &data_off, &S) == ST_OK) break;
            if ((uint64_t)got >= fsize) return ST_E_FORMAT;
        }
    }
    if (!has_range) qstart = qend = 0;
    const uint32_t qidx = vcfc_idx::ref_to_idx(qref, qref_len);
    vcfc_idx::Entry ent;
    if (lookup(I, qstart, qend, &ent)) return ST_OK;
    uint64_t p = ent.off;
    if (p >= fsize) return ST_OK;
    if (p < data_off) return ST_E_FORMAT;
    uint64_t window = std::max<uint64_t>(window_bytes, 64);
    std::vector<uint64_t> rec;
    while (p < fsize) {
        const uint64_t want = std::min(window, fsize - p);
        uint8_t *hbuf = B.host(Buffers::HOST_IN, want + 64);
        if (!hbuf) return ST_E_HIP;
        const int64_t got = R.read(hbuf, p, want);
        if (got < 0) return ST_E_IO;
        if (stats) { stats->windows++; stats->bytes += (uint64_t)got; }
        const bool eof = (uint64_t)got < want || p + (uint64_t)got >= fsize;
        const int why = vcfc_idx::hop_why(hbuf, (uint64_t)got, rec);
        const uint64_t nrec = rec.size() - 1;
        if (!nrec) {
            if (why == vcfc_idx::HOP_BAD || eof || window >= (1ull << 31)) return ST_E_FORMAT;   // not a record start
            window *= 2;   // one record larger than the window
            continue;
        }
        if (stats) stats->records += nrec;
        const uint8_t *d_in = vcfc_dec::upload(B, Buffers::IN, hbuf, (uint64_t)got, s);
        const uint64_t *d_rec = reinterpret_cast<const uint64_t *>(
            vcfc_dec::upload(B, Buffers::REC, reinterpret_cast<const uint8_t *>(rec.data()), 8 * (nrec + 1), s));
        const VcfcSparseIndexLayout L = vcfc_sparse_index_workspace_layout(nrec);
        uint8_t *ws = static_cast<uint8_t *>(B.get(Buffers::WS, L.total));
        uint8_t *d_flag = static_cast<uint8_t *>(B.get(Buffers::FLAG, nrec + 64));
        uint64_t *d_small = static_cast<uint64_t *>(B.get(Buffers::SMALL, 64));
        if (!d_in || !d_rec || !ws || !d_flag || !d_small) return ST_E_HIP;
        uint8_t *d_ref = ws + L.ref_idx;
        uint64_t *d_pos = reinterpret_cast<uint64_t *>(ws + L.pos);
        uint64_t words[2] = {VCFCD_NO_ERROR, ~0ull};   // first failing record, first record after the query
        if (vcfc_sparse_index_span(d_in, d_rec, nrec, 1, d_ref, d_pos, d_small, s) != hipSuccess ||
            vcfc_index_compare(d_ref, d_pos, d_pos, nrec, qidx, qstart, qend, d_flag, d_small + 1, s) != hipSuccess ||
            hipMemcpyAsync(words, d_small, 16, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
        const uint64_t bad = words[0] == VCFCD_NO_ERROR ? ~0ull : words[0] >> 8;
        const uint64_t stop_at = std::min(std::min(bad, words[1]), nrec);   // the walk ends before this record
        for (uint64_t j0 = 0; j0 < stop_at;) {
            int stop = 0;
            uint64_t cont = 0;
            std::vector<uint64_t> lend;
            const int st = vcfc_dec::decode_records(d_in, (uint64_t)got, S, d_rec + j0, d_flag + j0, stop_at - j0, B, s,
                                                    sink, out_batch, &stop, &cont, &lend);
            if (st) return st;
            if (stop == 1) return ST_E_FORMAT;
            if (stop == 0) break;
            j0 += lend.size();
        }
        if (stop_at < nrec) return bad <= words[1] ? ST_E_FORMAT : ST_OK;   // (a failing record is never compared)
        p += rec[nrec];
    }
    return ST_OK;
}

// gap-analysis (gap_analysis, reference src/main.cpp:3931-3980) over a whole
// .vcfc (host bytes): one text line "<POS> <decoded line bytes> <compressed
// count>\n" per record, in order.  The exact decode plan sizes the lines
// without writing them; vcfc_gap_fields locates the POS text and gives the
// reference's count; the host formats.  Where the decoder refuses a record
// the lines before it are sunk: ST_E_FORMAT, *err_record = the record.
inline int gap_analysis(const uint8_t *h_in, uint64_t n_bytes, Buffers &B, hipStream_t s, const Sink &sink,
                        int64_t *err_record) {
    if (err_record) *err_record = -1;
    uint64_t data_off = 0, S = 0;
    int st = vcfc_dec::parse_header(h_in, n_bytes, &data_off, &S);
    if (st) return st;
    const uint8_t *data = h_in + data_off;
    std::vector<uint64_t> rec;
    const int why = vcfc_idx::hop_why(data, n_bytes - data_off, rec);
    const uint64_t nrec = rec.size() - 1;
    uint64_t stop = why != vcfc_idx::HOP_END ? nrec : ~0ull;
    if (nrec) {
        const uint8_t *d_in = vcfc_dec::upload(B, Buffers::IN, data, rec[nrec], s);
        const uint64_t *d_rec = reinterpret_cast<const uint64_t *>(
            vcfc_dec::upload(B, Buffers::REC, reinterpret_cast<const uint8_t *>(rec.data()), 8 * (nrec + 1), s));
        const VcfcDecodeLayout L = vcfc_decode_workspace_layout(nrec);
        uint8_t *ws = static_cast<uint8_t *>(B.get(Buffers::WS, L.total));
        uint64_t *d_loff = static_cast<uint64_t *>(B.get(Buffers::LINE_OFF, 8 * (nrec + 1)));
        // pos_off (8 n), ccount (8 n), pos_len (4 n)
        uint8_t *d_gap = static_cast<uint8_t *>(B.get(Buffers::OUT, 20 * nrec + 64));
        if (!d_in || !d_rec || !ws || !d_loff || !d_gap) return ST_E_HIP;
        uint64_t *d_po = reinterpret_cast<uint64_t *>(d_gap), *d_cc = d_po + nrec;
        uint32_t *d_pl = reinterpret_cast<uint32_t *>(d_cc + nrec);
        VcfcDecodeArgs a;
        a.in = d_in; a.n_bytes = rec[nrec]; a.rec_start = d_rec; a.select = nullptr; a.n = nrec; a.S = S;
        a.out = nullptr; a.out_cap = 0; a.line_off = d_loff;
        a.st = reinterpret_cast<uint32_t *>(ws + L.st);
        a.line_size = reinterpret_cast<uint32_t *>(ws + L.line_size);
        a.end = reinterpret_cast<uint64_t *>(ws + L.end);
        a.seq_list = reinterpret_cast<uint32_t *>(ws + L.seq_list);
        a.seq_count = reinterpret_cast<uint32_t *>(ws + L.seq_count);
        a.err = reinterpret_cast<uint64_t *>(ws + L.err);
        a.partials = reinterpret_cast<uint64_t *>(ws + L.partials);
        uint64_t err = VCFCD_NO_ERROR;
        if (vcfc_decode_plan(a, true, s) != hipSuccess ||
            vcfc_gap_fields(d_in, d_rec, nrec, S, d_po, d_pl, d_cc, a.err, s) != hipSuccess ||
            hipMemcpyAsync(&err, a.err, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
        if (err != VCFCD_NO_ERROR) stop = std::min(stop, err >> 8);
        const uint64_t upto = std::min(stop, nrec);
        std::vector<uint64_t> loff(upto + 1), po(upto), cc(upto);
        std::vector<uint32_t> pl(upto);
        if (upto) {
            if (hipMemcpyAsync(loff.data(), d_loff, 8 * (upto + 1), hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(po.data(), d_po, 8 * upto, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(cc.data(), d_cc, 8 * upto, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(pl.data(), d_pl, 4 * upto, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess)
                return ST_E_HIP;
        }
        std::vector<uint8_t> text;
        text.reserve(1 << 20);
        char num[48];
        for (uint64_t i = 0; i < upto; i++) {
            text.insert(text.end(), data + po[i], data + po[i] + pl[i]);   // POS verbatim, not re-formatted
            const int k = snprintf(num, sizeof(num), " %llu %llu\n", (unsigned long long)(loff[i + 1] - loff[i]),
                                   (unsigned long long)cc[i]);
            text.insert(text.end(), num, num + k);
            if (text.size() >= (1 << 20) - 64) {
                if (!sink(text.data(), text.size())) return ST_E_IO;
                text.clear();
            }
        }
        if (!text.empty() && !sink(text.data(), text.size())) return ST_E_IO;
    }
    if (stop != ~0ull) {
        if (err_record) *err_record = (int64_t)stop;
        return ST_E_FORMAT;
    }
    return ST_OK;
}

}  // namespace vcfc_spx
