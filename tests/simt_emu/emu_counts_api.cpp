// TEST INFRASTRUCTURE ONLY: C entry points that run the genotype-counts
// kernels (csrc/vcfc_counts.hip) and their host driver
// (csrc/vcfc_counts_driver.h) on the fiber emulator, with host memory
// standing in for HBM.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vcfc_device.h"
#include "vcfc_counts_driver.h"
#include "emu.h"
#include "host_buffers.h"

extern "C" uint64_t emu_counts_lds_samples() { return VCFC_COUNTS_LDS_SAMPLES; }
extern "C" uint64_t emu_counts_trip_records(uint64_t S, int with_sample_table) {
    return vcfc_counts_scan_trip(S, with_sample_table != 0);
}
extern "C" uint64_t emu_counts_workspace_size(uint64_t n, uint64_t S) { return vcfc_counts_workspace_layout(n, S).total; }

// genotype-counts over a whole .vcfc (the C ABI's control flow): rows and
// indices up to rows_cap, the sample table (5 S words) on status 0; the two
// renderings where the header was accepted
extern "C" int emu_counts_file(const uint8_t *in, uint64_t n, int has_query, const uint8_t *ref, uint64_t ref_len,
                               int has_range, uint64_t qstart, uint64_t qend, uint64_t rec_batch, uint64_t *index,
                               uint32_t *rows, uint64_t rows_cap, uint64_t *n_rows, uint64_t *samples, uint64_t *n_samples,
                               uint64_t *err_record, uint8_t *vtext, uint64_t *vtext_len, uint8_t *stext,
                               uint64_t *stext_len, uint64_t text_cap) {
    *n_rows = *n_samples = *vtext_len = *stext_len = 0;
    *err_record = ~0ull;
    const vcfc_cnt::Query q{ref, ref_len, has_range, qstart, qend};
    vcfc_cnt::Result R;
    uint64_t data_off = 0, S = 0;
    HostBuffers B;
    const int st = vcfc_cnt::counts_file(in, n, has_query ? &q : nullptr, B, nullptr, R, &data_off, &S, rec_batch);
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
    if (data_off && S) {
        std::vector<uint8_t> text;
        vcfc_cnt::render_variants(in + data_off, R, text);
        if (text.size() > text_cap) return 4;
        memcpy(vtext, text.data(), text.size());
        *vtext_len = text.size();
        if (st == vcfc_cnt::ST_OK) {
            vcfc_cnt::render_samples(in, data_off, S, R, text);
            if (text.size() > text_cap) return 4;
            memcpy(stext, text.data(), text.size());
            *stext_len = text.size();
        }
    }
    return st;
}

// the device entry (the C ABI's vcfc_genotype_counts_device, argument for
// argument) on records [rec[0], rec[n])
extern "C" int emu_counts_device(const uint8_t *recs, const uint64_t *rec, const uint8_t *select, uint64_t n, uint64_t S,
                                 uint32_t *variant, uint64_t *sample, uint8_t *ws, uint64_t ws_bytes, uint64_t *err) {
    HostInput in(recs, n && rec ? rec[n] : 0);
    return vcfc_cnt::counts_device(recs ? in.p : nullptr, n && rec ? rec[n] : 0, rec, select, n, S, variant, sample, ws,
                                   ws_bytes, err, nullptr);
}
