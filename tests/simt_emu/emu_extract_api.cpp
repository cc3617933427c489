// TEST INFRASTRUCTURE ONLY: C entry points that run the extract kernels
// (csrc/vcfc_extract.hip) and their host driver (csrc/vcfc_extract_driver.h) on
// the fiber emulator, with host memory standing in for HBM.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vcfc_device.h"
#include "vcfc_extract_driver.h"
#include "vcfc_regions_driver.h"
#include "emu.h"
#include "host_buffers.h"

extern "C" uint64_t emu_extract_bound(uint64_t in_bytes, uint64_t n_records, uint64_t K) {
    return vcfc_ext::extract_bound(in_bytes, n_records, K);
}
extern "C" uint64_t emu_extract_tile(void) { return VCFC_EXTRACT_TILE; }
extern "C" uint64_t emu_extract_workspace_size(uint64_t n, uint64_t K) { return vcfc_extract_workspace_layout(n, K).total; }

static uint64_t g_sink_calls = 0;   // pieces the last emu_extract sank (header included)
extern "C" uint64_t emu_extract_sink_calls() { return g_sink_calls; }

extern "C" int emu_regions_build(const char *text, uint64_t len, uint8_t *table, uint64_t cap, uint64_t *bytes,
                                 uint64_t *n_regions, uint64_t *bad_line) {
    return vcfc_reg::regions_build(text, len, table, cap, bytes, n_regions, bad_line);
}

// extract over a whole .vcfc (the C ABI's control flow).  cols == nullptr and
// K == 0: all columns.  mode 0: no query; 1: one region (ref, has_range,
// start, end); 2: a region table.
extern "C" int emu_extract(const uint8_t *in, uint64_t n, const uint32_t *cols, uint64_t K, int mode, const uint8_t *ref,
                           uint64_t ref_len, int has_range, uint64_t qstart, uint64_t qend, const uint8_t *table,
                           uint64_t table_bytes, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t out_batch) {
    *out_len = 0;
    if (mode == 2 && !vcfc_reg::regions_validate(table, table_bytes)) return vcfc_ext::ST_E_ARG;
    vcfc_ext::Call c;
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
    VcfcQuery q;
    const uint8_t *d_table = nullptr;
    vcfc_dec::MatchStep m;
    if (mode == 1) m = vcfc_dec::region_step(ref, ref_len, has_range, qstart, qend, &q);
    if (mode == 2) m = vcfc_reg::regions_step(table, table_bytes, &d_table);
    st = vcfc_ext::extract_section(in + c.data_off, n - c.data_off, c.S, c.csort, c.rank, mode ? &m : nullptr, B, nullptr,
                                   sink, out_batch);
    *out_len = o;
    return st;
}

// the device entry's kernels on records[rec[0], rec[n]): plan + write in one
// go; out has out_cap bytes (+ the caller's canary), *err the error word
extern "C" int emu_extract_device(const uint8_t *recs, const uint64_t *rec, const uint8_t *select, uint64_t n, uint64_t S,
                                  const uint32_t *cols, uint64_t K, uint8_t *out, uint64_t out_cap, uint64_t *rec_off,
                                  uint64_t *err) {
    std::vector<uint32_t> csort, rank;
    if (vcfc_ext::device_columns(cols, K, S, csort, rank)) return vcfc_ext::ST_E_ARG;
    std::vector<uint8_t> ws(vcfc_extract_workspace_layout(n, csort.size()).total + 64, 0xCD);
    HostInput in(recs, n ? rec[n] : 0);
    return vcfc_sub::records_device(vcfc_ext::EXTRACT, in.p, n ? rec[n] : 0, rec, select, n, S, csort, rank, out, out_cap,
                                    rec_off, ws.data(), ws.size(), err, nullptr);
}
