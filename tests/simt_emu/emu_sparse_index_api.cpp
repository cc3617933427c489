// TEST INFRASTRUCTURE ONLY: C entry points that run the sparse-index kernels
// (csrc/vcfc_sparse_index.hip) and their host drivers
// (csrc/vcfc_sparse_index_driver.h) on the fiber emulator, with host memory
// standing in for HBM and an in-memory block map standing in for the sparse
// index file.
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "vcfc_device.h"
#include "vcfc_sparse_index_driver.h"
#include "emu.h"
#include "host_buffers.h"

namespace {
constexpr uint64_t BLK = 4096;
// a sparse file of 4 KiB blocks: written blocks are data, the rest are holes
struct BlockFile : vcfc_spx::Writer, vcfc_spx::IndexFile {
    std::map<uint64_t, std::array<uint8_t, BLK>> blocks;
    uint64_t size = 0, limit = 1ull << 63, writes = 0, reads = 0, seeks = 0;
    int pwrite(const uint8_t *p, uint64_t k, uint64_t off) override {
        if (off >= limit || off + k > limit) return 1;
        writes++;
        for (uint64_t i = 0; i < k; i++) {
            auto it = blocks.find((off + i) / BLK);
            if (it == blocks.end()) it = blocks.emplace((off + i) / BLK, std::array<uint8_t, BLK>{}).first;
            it->second[(off + i) % BLK] = p[i];
        }
        size = std::max(size, off + k);
        return 0;
    }
    int64_t pread(uint8_t *dst, uint64_t off, uint64_t k) override {
        reads++;
        if (off >= size) return 0;
        k = std::min(k, size - off);
        for (uint64_t i = 0; i < k; i++) {
            auto it = blocks.find((off + i) / BLK);
            dst[i] = it == blocks.end() ? 0 : it->second[(off + i) % BLK];
        }
        return (int64_t)k;
    }
    int64_t seek_data(uint64_t off) override {
        seeks++;
        if (off >= size) return -1;
        auto it = blocks.lower_bound(off / BLK);
        if (it == blocks.end()) return -1;
        return (int64_t)std::max(off, it->first * BLK);
    }
};

// reads of the queried file, logged as (offset, bytes) pairs
struct LogReader : vcfc_idx::Reader {
    const uint8_t *p;
    uint64_t n;
    uint64_t *log, cap, used = 0;
    uint64_t size() const override { return n; }
    int64_t read(uint8_t *dst, uint64_t off, uint64_t k) override {
        if (off >= n) k = 0;
        k = std::min(k, n - std::min(off, n));
        if (log && used < cap) { log[2 * used] = off; log[2 * used + 1] = k; }
        used++;
        if (k) memcpy(dst, p + off, k);
        return (int64_t)k;
    }
};
}  // namespace

// vcfc_spx::create_index over a whole .vcfc.  slots: (offset, 13 bytes) of
// every non-zero 256-byte slot, ascending; info = {slots, apparent size,
// pwrite calls, record-by-record path taken, entries written}.  limit: the
// first offset the "file system" refuses.
extern "C" int emu_spx_create(const uint8_t *in, uint64_t n, uint64_t limit, uint64_t *slot_off, uint8_t *slot_ent,
                              uint64_t cap, uint64_t *info, int64_t *err_record, int *seek_failed) {
    HostBuffers B;
    BlockFile F;
    F.limit = limit;
    vcfc_spx::CreateStats cs;
    const int st = vcfc_spx::create_index(in, n, B, nullptr, F, err_record, seek_failed, &cs);
    uint64_t k = 0;
    static const uint8_t zero[13] = {0};
    for (const auto &b : F.blocks)
        for (uint64_t o = 0; o < BLK; o += 256) {
            if (!memcmp(b.second.data() + o, zero, 13)) continue;
            if (k < cap) {
                slot_off[k] = b.first * BLK + o;
                memcpy(slot_ent + 13 * k, b.second.data() + o, 13);
            }
            k++;
        }
    info[0] = k; info[1] = F.size; info[2] = F.writes; info[3] = (uint64_t)cs.in_order; info[4] = cs.entries;
    return k > cap ? 4 : st;
}

// vcfc_spx::query_index against an index given as its non-zero slots and its
// apparent size.  log: (offset, bytes) of every read of the .vcfc, *log_n
// their count; idx_io = {preads, SEEK_DATA calls} on the index
extern "C" int emu_spx_query(const uint8_t *in, uint64_t n, const uint64_t *slot_off, const uint8_t *slot_ent,
                             uint64_t slots, uint64_t index_size, const uint8_t *ref, uint64_t ref_len, int has_range,
                             uint64_t qstart, uint64_t qend, uint8_t *out, uint64_t cap, uint64_t *out_len,
                             uint64_t window_bytes, uint64_t out_batch, uint64_t *log, uint64_t log_cap,
                             uint64_t *log_n, uint64_t *idx_io) {
    BlockFile F;
    for (uint64_t k = 0; k < slots; k++) F.pwrite(slot_ent + 13 * k, 13, slot_off[k]);
    F.size = index_size;
    F.reads = F.seeks = 0;
    uint64_t o = 0;
    auto sink = [&](const uint8_t *p, uint64_t k) {
        if (o + k > cap) return false;
        memcpy(out + o, p, k);
        o += k;
        return true;
    };
    LogReader R;
    R.p = in; R.n = n; R.log = log; R.cap = log_cap;
    HostBuffers B;
    const int st = vcfc_spx::query_index(R, F, ref, ref_len, has_range, qstart, qend, B, nullptr, sink, window_bytes,
                                         nullptr, out_batch);
    *out_len = o;
    if (log_n) *log_n = R.used;
    if (idx_io) { idx_io[0] = F.reads; idx_io[1] = F.seeks; }
    return st;
}

// vcfc_sparse_index_build on records[rec[0], rec[n]) behind a guard page;
// words = {err, count, status[0], status[1], status[2]}
extern "C" int emu_spx_device(const uint8_t *recs, const uint64_t *rec, uint64_t n, uint64_t base, uint8_t *entries,
                              uint64_t *file_off, uint64_t *words) {
    const VcfcSparseIndexLayout L = vcfc_sparse_index_workspace_layout(n);
    std::vector<uint8_t> ws(L.total + 64, 0xCD);
    HostInput g(recs, n ? rec[n] : 0, true);   // behind a guard page (host_buffers.h)
    for (int k = 0; k < 5; k++) words[k] = 0xCDCDCDCDCDCDCDCDull;
    return (int)vcfc_sparse_index_build(g.p, rec, n, base, entries, file_off, words + 1, words + 2, ws.data(), L, words,
                                        nullptr);
}

// vcfc_sparse_index_span on records behind a guard page
extern "C" int emu_spx_span(const uint8_t *recs, const uint64_t *rec, uint64_t n, int walk, uint8_t *ref_idx,
                            uint64_t *pos, uint64_t *err) {
    HostInput g(recs, n ? rec[n] : 0, true);   // behind a guard page (host_buffers.h)
    return (int)vcfc_sparse_index_span(g.p, rec, n, walk, ref_idx, pos, err, nullptr);
}

// The device entry vcfc_decode_sizes_device, step for step as csrc/vcfc_api.cpp
// takes it: the exact plan without the write, then the gap fields.
extern "C" int emu_decode_sizes(const uint8_t *recs, uint64_t in_bytes, const uint64_t *rec, uint64_t n, uint64_t S,
                                uint64_t *line_off, uint64_t *pos_off, uint32_t *pos_len, uint64_t *ccount,
                                uint64_t *err) {
    const VcfcDecodeLayout L = vcfc_decode_workspace_layout(n);
    std::vector<uint8_t> ws(L.total + 64, 0xCD);
    HostInput in(recs, in_bytes);
    VcfcDecodeArgs a;
    a.in = in.p; a.n_bytes = in_bytes; a.rec_start = rec; a.select = nullptr; a.n = n; a.S = S;
    a.out = nullptr; a.out_cap = 0; a.line_off = line_off;
    a.st = reinterpret_cast<uint32_t *>(ws.data() + L.st);
    a.line_size = reinterpret_cast<uint32_t *>(ws.data() + L.line_size);
    a.end = reinterpret_cast<uint64_t *>(ws.data() + L.end);
    a.seq_list = reinterpret_cast<uint32_t *>(ws.data() + L.seq_list);
    a.seq_count = reinterpret_cast<uint32_t *>(ws.data() + L.seq_count);
    a.err = err;
    a.partials = reinterpret_cast<uint64_t *>(ws.data() + L.partials);
    if (vcfc_decode_plan(a, true, nullptr) != hipSuccess) return 3;
    return vcfc_gap_fields(in.p, rec, n, S, pos_off, pos_len, ccount, err, nullptr) == hipSuccess ? 0 : 3;
}

// vcfc_spx::gap_analysis over a whole .vcfc: the text of start-positions.txt
extern "C" int emu_spx_gap(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len,
                           int64_t *err_record) {
    uint64_t o = 0;
    auto sink = [&](const uint8_t *p, uint64_t k) {
        if (o + k > cap) return false;
        memcpy(out + o, p, k);
        o += k;
        return true;
    };
    HostBuffers B;
    const int st = vcfc_spx::gap_analysis(in, n, B, nullptr, sink, err_record);
    *out_len = o;
    return st;
}
