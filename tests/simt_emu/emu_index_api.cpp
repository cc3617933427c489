// TEST INFRASTRUCTURE ONLY: C entry points that run the binned-index kernels
// (csrc/vcfc_index.hip) and their host drivers (csrc/vcfc_index_driver.h) on
// the fiber emulator, with host memory standing in for HBM.
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vcfc_device.h"
#include "vcfc_index_driver.h"
#include "emu.h"
#include "host_buffers.h"

namespace {
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

// vcfc_idx::create_index over a whole .vcfc
extern "C" int emu_index_create(const uint8_t *in, uint64_t n, uint64_t E, uint8_t *out, uint64_t cap,
                                uint64_t *out_len, int64_t *err_record) {
    HostBuffers B;
    std::vector<uint8_t> idx;
    const int st = vcfc_idx::create_index(in, n, E, B, nullptr, idx, err_record);
    *out_len = idx.size();
    if (idx.size() > cap) return 4;
    if (!idx.empty()) memcpy(out, idx.data(), idx.size());
    return st;
}

// vcfc_idx::query_index; log: (offset, bytes) of every read of the file, *log_n their count
extern "C" int emu_index_query(const uint8_t *in, uint64_t n, const uint8_t *index, uint64_t index_bytes,
                               const uint8_t *ref, uint64_t ref_len, int has_range, uint64_t qstart, uint64_t qend,
                               uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t window_bytes, uint64_t out_batch,
                               uint64_t *log, uint64_t log_cap, uint64_t *log_n) {
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
    const int st = vcfc_idx::query_index(R, index, index_bytes, ref, ref_len, has_range, qstart, qend, B, nullptr, sink,
                                         window_bytes, nullptr, out_batch);
    *out_len = o;
    if (log_n) *log_n = R.used;
    return st;
}

// vcfc_index_build on records[rec[0], rec[n]) behind a guard page; words = {err, count, largest end}
extern "C" int emu_index_device(const uint8_t *recs, const uint64_t *rec, uint64_t n, uint64_t base, uint64_t E,
                                uint8_t *entries, uint64_t entries_cap, uint64_t *words) {
    const VcfcIndexLayout L = vcfc_index_workspace_layout(n);
    std::vector<uint8_t> ws(L.total + 64, 0xCD);
    HostInput g(recs, n ? rec[n] : 0, true);   // behind a guard page (host_buffers.h)
    words[0] = words[1] = words[2] = 0xCDCDCDCDCDCDCDCDull;
    return (int)vcfc_index_build(g.p, rec, n, base, E, entries, entries_cap, words + 1, words + 2, ws.data(), L, words,
                                 nullptr);
}

// vcfc_index_span on records behind a guard page
extern "C" int emu_record_span(const uint8_t *recs, const uint64_t *rec, uint64_t n, uint8_t *ref_idx, uint64_t *pos,
                               uint64_t *end, uint64_t *err) {
    HostInput g(recs, n ? rec[n] : 0, true);   // behind a guard page (host_buffers.h)
    return (int)vcfc_index_span(g.p, rec, n, ref_idx, pos, end, err, nullptr);
}

// vcfc_index_compare on host arrays
extern "C" int emu_index_compare(const uint8_t *ref_idx, const uint64_t *pos, const uint64_t *end, uint64_t n,
                                 uint32_t qidx, uint64_t qstart, uint64_t qend, uint8_t *flag, uint64_t *first_after) {
    return (int)vcfc_index_compare(ref_idx, pos, end, n, qidx, qstart, qend, flag, first_after, nullptr);
}
