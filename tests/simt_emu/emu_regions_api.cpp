// TEST INFRASTRUCTURE ONLY: C entry points that run the region-list kernel
// (csrc/vcfc_regions.hip), its host side (csrc/vcfc_regions_driver.h) and the
// three drivers that take its match step on the fiber emulator, with host
// memory standing in for HBM.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vcfc_device.h"
#include "vcfc_counts_driver.h"
#include "vcfc_regions_driver.h"
#include "vcfc_subset_driver.h"
#include "emu.h"
#include "host_buffers.h"

namespace {
struct OutSink {
    uint8_t *out;
    uint64_t cap, o = 0;
    bool operator()(const uint8_t *p, uint64_t k) {
        if (o + k > cap) return false;
        memcpy(out + o, p, k);
        o += k;
        return true;
    }
};
}  // namespace

extern "C" int emu_regions_build(const char *text, uint64_t len, uint8_t *table, uint64_t cap, uint64_t *bytes,
                                 uint64_t *n_regions, uint64_t *bad_line) {
    return vcfc_reg::regions_build(text, len, table, cap, bytes, n_regions, bad_line);
}

extern "C" uint64_t emu_regions_workspace_size(uint64_t table_bytes) { return vcfc_reg::regions_workspace_size(table_bytes); }

extern "C" int emu_regions_upload(const uint8_t *table, uint64_t bytes, void *ws, uint64_t ws_bytes) {
    return vcfc_reg::regions_upload(table, bytes, ws, ws_bytes, nullptr);
}

// the device entry (the C ABI's vcfc_regions_match_device, argument for
// argument) on records [rec[0], rec[n])
extern "C" int emu_regions_match(const uint8_t *recs, const uint64_t *rec, uint64_t n, const void *ws, uint64_t ws_bytes,
                                 uint8_t *flag, uint64_t *err) {
    HostInput in(recs, n ? rec[n] : 0);
    return vcfc_reg::regions_match_device(in.p, rec, n, ws, ws_bytes, flag, err, nullptr);
}

// the one-region match (the C ABI's vcfc_query_match_device) on the same records
extern "C" int emu_regions_query_match(const uint8_t *recs, const uint64_t *rec, uint64_t n, const uint8_t *ref,
                                       uint64_t ref_len, int has_range, uint64_t start, uint64_t end, uint8_t *flag,
                                       uint64_t *err) {
    HostInput in(recs, n ? rec[n] : 0);
    VcfcQuery q;
    q.ref = ref; q.ref_len = (uint32_t)ref_len; q.has_range = has_range ? 1u : 0u; q.start = start; q.end = end;
    return vcfc_query_match(in.p, rec, n, q, flag, err, nullptr) == hipSuccess ? 0 : vcfc_reg::ST_E_HIP;
}

// query-regions over a whole .vcfc (the C ABI's control flow)
extern "C" int emu_regions_query(const uint8_t *in, uint64_t n, const uint8_t *table, uint64_t table_bytes, uint8_t *out,
                                 uint64_t cap, uint64_t *out_len, uint64_t out_batch) {
    *out_len = 0;
    if (!vcfc_reg::regions_validate(table, table_bytes)) return vcfc_reg::ST_E_ARG;
    uint64_t data_off = 0, S = 0;
    int st = vcfc_dec::parse_header(in, n, &data_off, &S);
    if (st) return st;
    OutSink sink{out, cap};
    const uint8_t *d_table = nullptr;
    HostBuffers B;
    st = vcfc_dec::query_regions_section(in + data_off, n - data_off, S, vcfc_reg::regions_step(table, table_bytes, &d_table),
                                         B, nullptr, std::ref(sink), out_batch);
    *out_len = sink.o;
    return st;
}

// query-samples-regions over a whole .vcfc
extern "C" int emu_regions_query_samples(const uint8_t *in, uint64_t n, const uint8_t *table, uint64_t table_bytes,
                                         const uint32_t *cols, uint64_t K, uint8_t *out, uint64_t cap, uint64_t *out_len,
                                         uint64_t out_batch) {
    *out_len = 0;
    if (!vcfc_reg::regions_validate(table, table_bytes)) return vcfc_reg::ST_E_ARG;
    vcfc_sub::Call c;
    int st = c.prepare(in, n, cols, K);
    if (st) return st;
    OutSink sink{out, cap};
    const uint8_t *d_table = nullptr;
    HostBuffers B;
    st = vcfc_sub::matched_section(in + c.data_off, n - c.data_off, c.S, c.csort, c.rank,
                                   vcfc_reg::regions_step(table, table_bytes, &d_table), B, nullptr, std::ref(sink), out_batch);
    *out_len = sink.o;
    return st;
}

// genotype-counts-regions over a whole .vcfc: rows and indices up to
// rows_cap, the sample table (5 S words) on status 0
extern "C" int emu_regions_counts(const uint8_t *in, uint64_t n, const uint8_t *table, uint64_t table_bytes,
                                  uint64_t rec_batch, uint64_t *index, uint32_t *rows, uint64_t rows_cap, uint64_t *n_rows,
                                  uint64_t *samples, uint64_t *n_samples, uint64_t *err_record) {
    *n_rows = *n_samples = 0;
    *err_record = ~0ull;
    if (!vcfc_reg::regions_validate(table, table_bytes)) return vcfc_reg::ST_E_ARG;
    const uint8_t *d_table = nullptr;
    const vcfc_dec::MatchStep match = vcfc_reg::regions_step(table, table_bytes, &d_table);
    vcfc_cnt::Result R;
    uint64_t data_off = 0, S = 0;
    HostBuffers B;
    const int st = vcfc_cnt::counts_file(in, n, &match, B, nullptr, R, &data_off, &S, rec_batch);
    if (st != vcfc_cnt::ST_OK && st != vcfc_cnt::ST_E_FORMAT) return st;
    *err_record = R.err_record;
    *n_rows = R.index.size();
    if (*n_rows > rows_cap) return 4;
    std::copy(R.index.begin(), R.index.end(), index);
    std::copy(R.rows.begin(), R.rows.end(), rows);
    if (st == vcfc_cnt::ST_OK) {
        *n_samples = S;
        std::copy(R.samples.begin(), R.samples.end(), samples);
    }
    return st;
}
