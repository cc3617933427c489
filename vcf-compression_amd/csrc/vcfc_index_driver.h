// vcfc_index_driver.h -- host drivers of the binned external index, shared by
// the C ABI (vcfc_api.cpp) and the CPU emulator harness
// (tests/simt_emu/emu_index_api.cpp), so the same control flow is tested on
// both.
//
// create (create_binned_index4, reference src/main.cpp:1284-1637):
//   1. parse the header, hop the LEN headers on the host;
//   2. upload the data section; vcfc_index_build computes every record's
//      span, the prefix maximum of the end positions, the open flags and the
//      packed entries on the GPU;
//   3. where some end position is 2^32 or more the reference compares a
//      64-bit value with the entry's truncated u32 and the parallel form no
//      longer holds: the sequential rule is replayed on the host from the
//      GPU's end array.
// query (query_binned_index_binarysearch, :2974-3349):
//   1. the reference's binary search over the index on the host;
//   2. from the entry's byte_offset the file is read in windows; per window:
//      hop, k_index_span, k_index_compare, decode_records with the flags;
//   3. stop at the window holding the first record after the query, or EOF.
#pragma once
#include "vcfc_decode_driver.h"

namespace vcfc_idx {

using vcfc_dec::Buffers;
using vcfc_dec::Sink;
constexpr int ST_OK = 0, ST_E_ARG = 5, ST_E_HIP = 6, ST_E_IO = 7, ST_E_FORMAT = 8;   // = include/vcfc.h codes
constexpr uint64_t ENTRY_BYTES = 13;   // {u8 ref_idx, u32 position, u64 byte_offset}, packed, little-endian

// reference_name_map (src/utils.hpp:97-100)
inline uint32_t ref_to_idx(const uint8_t *c, uint64_t n) {
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

// vcfc_dec::hop, and why it stopped at rec.back()
enum { HOP_END = 0, HOP_SHORT, HOP_BAD, HOP_BEYOND };   // all bytes used / < 8 left / header bits or LEN < 4 / LEN past the end
inline int hop_why(const uint8_t *in, uint64_t n, std::vector<uint64_t> &rec) {
    rec.clear();
    uint64_t p = 0;
    int why = HOP_END;
    while (p < n) {
        if (n - p < 8) { why = HOP_SHORT; break; }
        const uint8_t *h = in + p;
        if ((h[0] >> 6) != 3u || (h[4] >> 6) != 3u) { why = HOP_BAD; break; }
        const uint64_t L = ((uint64_t)(h[0] & 0x3Fu) << 24) | ((uint64_t)h[1] << 16) | ((uint64_t)h[2] << 8) | h[3];
        if (L < 4) { why = HOP_BAD; break; }
        if (L + 4 > n - p) { why = HOP_BEYOND; break; }
        rec.push_back(p);
        p += 4 + L;
    }
    rec.push_back(p);
    return why;
}

struct Entry {
    uint32_t ref;
    uint32_t pos;
    uint64_t off;
};
inline Entry get_entry(const uint8_t *idx, uint64_t j) {
    const uint8_t *e = idx + ENTRY_BYTES * j;
    Entry r;
    r.ref = e[0];
    r.pos = 0;
    r.off = 0;
    for (int k = 3; k >= 0; k--) r.pos = (r.pos << 8) | e[1 + k];
    for (int k = 7; k >= 0; k--) r.off = (r.off << 8) | e[5 + k];
    return r;
}
inline void put_entry(std::vector<uint8_t> &out, const Entry &x) {
    out.push_back((uint8_t)x.ref);
    for (int k = 0; k < 4; k++) out.push_back((uint8_t)(x.pos >> (8 * k)));
    for (int k = 0; k < 8; k++) out.push_back((uint8_t)(x.off >> (8 * k)));
}

// The reference's sequential rule (:1430-1482): record 0 opens an entry;
// record i with i % E == 0 opens one iff end_i > the last entry's (u32)
// position; every other record raises that position to end_i when larger.
inline void replay(const uint8_t *ref, const uint64_t *end, const uint64_t *rec, uint64_t n, uint64_t base, uint64_t E,
                   std::vector<uint8_t> &out) {
    std::vector<Entry> v;
    for (uint64_t i = 0; i < n; i++) {
        const Entry x{ref[i], (uint32_t)end[i], base + rec[i]};
        if (v.empty()) v.push_back(x);
        else if (i % E == 0) { if (end[i] > (uint64_t)v.back().pos) v.push_back(x); }
        else if (end[i] > (uint64_t)v.back().pos) v.back().pos = (uint32_t)end[i];
    }
    out.clear();
    out.reserve(ENTRY_BYTES * v.size());
    for (const Entry &x : v) put_entry(out, x);
}

// The index of a whole .vcfc (host bytes).  *err_record: the first record
// the reference throws on (ST_E_FORMAT), else -1.
inline int create_index(const uint8_t *h_in, uint64_t n_bytes, uint64_t E, Buffers &B, hipStream_t s,
                        std::vector<uint8_t> &out, int64_t *err_record) {
    out.clear();
    if (err_record) *err_record = -1;
    if (E == 0) return ST_E_ARG;   // (the reference dies of SIGFPE)
    uint64_t data_off = 0;
    int st = vcfc_dec::parse_header(h_in, n_bytes, &data_off, nullptr);
    if (st) return st;
    const uint8_t *data = h_in + data_off;
    const uint64_t n = n_bytes - data_off;
    std::vector<uint64_t> rec;
    const int why = hop_why(data, n, rec);
    const uint64_t nrec = rec.size() - 1;
    uint64_t words[3] = {VCFCD_NO_ERROR, 0, 0};   // err, count, largest end
    uint8_t *ws = nullptr;
    VcfcIndexLayout L = vcfc_index_workspace_layout(nrec);
    uint8_t *d_entries = nullptr;
    if (nrec) {
        const uint8_t *d_in = vcfc_dec::upload(B, Buffers::IN, data, rec[nrec], s);
        const uint64_t *d_rec = reinterpret_cast<const uint64_t *>(
            vcfc_dec::upload(B, Buffers::REC, reinterpret_cast<const uint8_t *>(rec.data()), 8 * (nrec + 1), s));
        ws = static_cast<uint8_t *>(B.get(Buffers::WS, L.total));
        d_entries = static_cast<uint8_t *>(B.get(Buffers::OUT, ENTRY_BYTES * nrec + 64));
        uint64_t *d_small = static_cast<uint64_t *>(B.get(Buffers::SMALL, 64));
        if (!d_in || !d_rec || !ws || !d_entries || !d_small) return ST_E_HIP;
        if (vcfc_index_build(d_in, d_rec, nrec, data_off, E, d_entries, nrec, d_small + 1, d_small + 2, ws, L, d_small,
                             s) != hipSuccess ||
            hipMemcpyAsync(words, d_small, 24, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
    }
    if (words[0] != VCFCD_NO_ERROR) {
        if (err_record) *err_record = (int64_t)(words[0] >> 8);
        return ST_E_FORMAT;
    }
    if (why != HOP_END) {   // a record header the reference cannot read
        if (err_record) *err_record = (int64_t)nrec;
        return ST_E_FORMAT;
    }
    if (!nrec) return ST_OK;
    if (words[2] > 0xFFFFFFFFull) {
        std::vector<uint8_t> ref(nrec);
        std::vector<uint64_t> end(nrec);
        if (hipMemcpyAsync(ref.data(), ws + L.ref_idx, nrec, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(end.data(), ws + L.end, 8 * nrec, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
        replay(ref.data(), end.data(), rec.data(), nrec, data_off, E, out);
        return ST_OK;
    }
    out.resize(ENTRY_BYTES * words[1]);
    if (hipMemcpyAsync(out.data(), d_entries, out.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return ST_E_HIP;
    return ST_OK;
}

// The binary search of :3047-3167 over (ref_idx, position) against (qidx,
// qstart): the entry used is the last one read, stepped back once when it
// lies after the query.  An index of one entry (where the reference reads an
// uninitialised struct) uses entry 0.  false: no entries.
inline bool search_index(const uint8_t *idx, uint64_t count, uint32_t qidx, uint64_t qstart, Entry *out) {
    if (!count) return false;
    auto after = [&](const Entry &e) { return e.ref > qidx || (e.ref == qidx && (uint64_t)e.pos > qstart); };
    int64_t lo = 0, hi = (int64_t)count - 1, mid = (lo + hi) / 2;
    Entry e = get_entry(idx, 0);
    while (lo < hi) {
        mid = (lo + hi) / 2;
        e = get_entry(idx, (uint64_t)mid);
        if (e.ref == qidx && (uint64_t)e.pos == qstart) break;
        if (after(e)) {
            if (mid == 0) break;
            hi = mid - 1;
        } else {
            lo = mid + 1;
        }
    }
    if (mid > 0 && after(e)) e = get_entry(idx, (uint64_t)(mid - 1));
    *out = e;
    return true;
}

// the .vcfc being queried: bytes [off, off + k), short only at EOF; -1 on a read error
struct Reader {
    virtual ~Reader() {}
    virtual uint64_t size() const = 0;
    virtual int64_t read(uint8_t *dst, uint64_t off, uint64_t k) = 0;
};

struct QueryStats {
    uint64_t windows = 0, bytes = 0, records = 0;
};

// Indexed range query: the lines of the records in (ref, start, end), from
// the entry the search picks.  No byte before that entry's byte_offset is
// read, apart from the header.  window_bytes: bytes read per step (grown
// while one record does not fit).
inline int query_index(Reader &R, const uint8_t *index, uint64_t index_bytes, const uint8_t *qref, uint64_t qref_len,
                       int has_range, uint64_t qstart, uint64_t qend, Buffers &B, hipStream_t s, const Sink &sink,
                       uint64_t window_bytes = 4ull << 20, QueryStats *stats = nullptr,
                       uint64_t out_batch = 1ull << 30) {
    const uint64_t fsize = R.size();
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
    if (index_bytes % ENTRY_BYTES) return ST_E_FORMAT;   // "Index size was not a multiple of entry size"
    if (!has_range) qstart = qend = 0;
    const uint32_t qidx = ref_to_idx(qref, qref_len);
    Entry ent;
    if (!search_index(index, index_bytes / ENTRY_BYTES, qidx, qstart, &ent)) return ST_OK;
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
        const int why = hop_why(hbuf, (uint64_t)got, rec);
        const uint64_t nrec = rec.size() - 1;
        if (!nrec) {
            if (why == HOP_BAD || eof || window >= (1ull << 31)) return ST_E_FORMAT;   // not a record start
            window *= 2;   // one record larger than the window
            continue;
        }
        if (stats) stats->records += nrec;
        const uint8_t *d_in = vcfc_dec::upload(B, Buffers::IN, hbuf, (uint64_t)got, s);
        const uint64_t *d_rec = reinterpret_cast<const uint64_t *>(
            vcfc_dec::upload(B, Buffers::REC, reinterpret_cast<const uint8_t *>(rec.data()), 8 * (nrec + 1), s));
        const VcfcIndexLayout L = vcfc_index_workspace_layout(nrec);
        uint8_t *ws = static_cast<uint8_t *>(B.get(Buffers::WS, L.total));
        uint8_t *d_flag = static_cast<uint8_t *>(B.get(Buffers::FLAG, nrec + 64));
        uint64_t *d_small = static_cast<uint64_t *>(B.get(Buffers::SMALL, 64));
        if (!d_in || !d_rec || !ws || !d_flag || !d_small) return ST_E_HIP;
        uint8_t *d_ref = ws + L.ref_idx;
        uint64_t *d_pos = reinterpret_cast<uint64_t *>(ws + L.pos), *d_end = reinterpret_cast<uint64_t *>(ws + L.end);
        uint64_t words[2] = {VCFCD_NO_ERROR, ~0ull};   // first failing record, first record after the query
        if (vcfc_index_span(d_in, d_rec, nrec, d_ref, d_pos, d_end, d_small, s) != hipSuccess ||
            vcfc_index_compare(d_ref, d_pos, d_end, nrec, qidx, qstart, qend, d_flag, d_small + 1, s) != hipSuccess ||
            hipMemcpyAsync(words, d_small, 16, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return ST_E_HIP;
        const uint64_t bad = words[0] == VCFCD_NO_ERROR ? ~0ull : words[0] >> 8;
        const uint64_t stop_at = std::min(std::min(bad, words[1]), nrec);   // the walk ends before this record
        // the selected records before it decode; a line whose parse ends off
        // its record is kept (the reference seeks to the LEN hop after it)
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

}  // namespace vcfc_idx
