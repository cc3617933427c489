// TEST INFRASTRUCTURE ONLY: C entry points that run the sample-subset kernels
// (csrc/vcfc_subset.hip) and their host driver (csrc/vcfc_subset_driver.h) on
// the fiber emulator, with host memory standing in for HBM.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vcfc_device.h"
#include "vcfc_subset_driver.h"
#include "emu.h"
#include "host_buffers.h"

using vcfc_sub::Call;

static uint64_t g_sink_calls = 0;   // pieces the last emu_subset_decompress sank (header included)
extern "C" uint64_t emu_subset_sink_calls() { return g_sink_calls; }
extern "C" uint64_t emu_subset_workspace_size(uint64_t n, uint64_t K) { return vcfc_subset_workspace_layout(n, K).total; }

// decompress-samples over a whole .vcfc (the C ABI's control flow)
extern "C" int emu_subset_decompress(const uint8_t *in, uint64_t n, const uint32_t *cols, uint64_t K, uint8_t *out,
                                     uint64_t cap, uint64_t *out_len, uint64_t out_batch) {
    *out_len = 0;
    Call c;
    int st = c.prepare(in, n, cols, K);
    if (st) return st;
    uint64_t o = 0;
    g_sink_calls = 0;
    auto sink = [&](const uint8_t *p, uint64_t k) {
        g_sink_calls++;
        if (o + k > cap) return false;
        memcpy(out + o, p, k);
        o += k;
        return true;
    };
    sink(c.hdr.data(), c.hdr.size());
    HostBuffers B;
    st = vcfc_sub::decode_section(in + c.data_off, n - c.data_off, c.S, c.csort, c.rank, B, nullptr, sink, out_batch);
    *out_len = o;
    return st;
}

// query-samples over a whole .vcfc
extern "C" int emu_subset_query(const uint8_t *in, uint64_t n, const uint8_t *ref, uint64_t ref_len, int has_range,
                                uint64_t qstart, uint64_t qend, const uint32_t *cols, uint64_t K, uint8_t *out,
                                uint64_t cap, uint64_t *out_len, uint64_t out_batch) {
    *out_len = 0;
    Call c;
    int st = c.prepare(in, n, cols, K);
    if (st) return st;
    uint64_t o = 0;
    auto sink = [&](const uint8_t *p, uint64_t k) {
        if (o + k > cap) return false;
        memcpy(out + o, p, k);
        o += k;
        return true;
    };
    HostBuffers B;
    st = vcfc_sub::query_section(in + c.data_off, n - c.data_off, c.S, c.csort, c.rank, ref, ref_len, has_range, qstart,
                                 qend, B, nullptr, sink, out_batch);
    *out_len = o;
    return st;
}

// the device entry's kernels on records[rec[0], rec[n]): plan + write in one
// go; out has out_cap bytes (+ the caller's canary), *err the error word
extern "C" int emu_subset_device(const uint8_t *recs, const uint64_t *rec, const uint8_t *select, uint64_t n, uint64_t S,
                                 const uint32_t *cols, uint64_t K, uint8_t *out, uint64_t out_cap, uint64_t *line_off,
                                 uint64_t *err) {
    std::vector<uint32_t> csort, rank;
    if (vcfc_sub::sort_columns(cols, K, S, csort, rank)) return vcfc_sub::ST_E_ARG;
    std::vector<uint8_t> ws(vcfc_subset_workspace_layout(n, K).total + 64, 0xCD);
    HostInput in(recs, n ? rec[n] : 0);
    return vcfc_sub::records_device(vcfc_sub::SUBSET, in.p, n ? rec[n] : 0, rec, select, n, S, csort, rank, out, out_cap,
                                    line_off, ws.data(), ws.size(), err, nullptr);
}

extern "C" int emu_sample_columns(const uint8_t *in, uint64_t n, const char *names, uint64_t names_len, uint32_t *cols,
                                  uint64_t cols_cap, uint64_t *n_cols, uint64_t *bad_off) {
    return vcfc_sub::sample_columns(in, n, names, names_len, cols, cols_cap, n_cols, bad_off);
}
