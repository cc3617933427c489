// TEST INFRASTRUCTURE ONLY: C entry points that run the genotype-matrix
// kernels (csrc/vcfc_matrix.hip) and their host driver
// (csrc/vcfc_matrix_driver.h) on the fiber emulator, with host memory
// standing in for HBM.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vcfc_device.h"
#include "vcfc_matrix_driver.h"
#include "vcfc_regions_driver.h"
#include "emu.h"
#include "host_buffers.h"

extern "C" uint64_t emu_matrix_row_bytes(int layout, uint64_t S) { return vcfc_matrix_row_size(layout, S); }
extern "C" uint64_t emu_matrix_lds_samples(int layout) { return vcfc_matrix_tile_samples(layout); }
extern "C" uint64_t emu_matrix_trip_records(int layout) { return vcfc_matrix_scan_trip(layout); }
extern "C" uint64_t emu_matrix_workspace_size(uint64_t n, uint64_t, int) { return vcfc_matrix_workspace_layout(n).total; }

// genotype-matrix over a whole .vcfc (the C ABI's control flow): indices and
// rows up to rows_cap; the three renderings of export-bed where the header was
// accepted (layout .bed only).  mode 0: every record, 1: one region, 2: a
// region table.
extern "C" int emu_matrix_file(const uint8_t *in, uint64_t n, int layout, int mode, const uint8_t *ref, uint64_t ref_len,
                               int has_range, uint64_t qstart, uint64_t qend, const uint8_t *table, uint64_t table_bytes,
                               uint64_t rec_batch, uint64_t *index, uint8_t *rows, uint64_t rows_cap, uint64_t *n_rows,
                               uint64_t *n_samples, uint64_t *err_record, uint8_t *bed, uint64_t *bed_len, uint8_t *bim,
                               uint64_t *bim_len, uint8_t *fam, uint64_t *fam_len, uint64_t text_cap) {
    *n_rows = *n_samples = *bed_len = *bim_len = *fam_len = 0;
    *err_record = ~0ull;
    std::vector<uint8_t> built;
    if (mode == 2) {   // `table` is region text: the table is built here
        uint64_t bytes = 0, n_regions = 0, bad_line = 0;
        built.resize(64 * table_bytes + 4096);
        if (vcfc_reg::regions_build(reinterpret_cast<const char *>(table), table_bytes, built.data(), built.size(), &bytes,
                                    &n_regions, &bad_line) != 0)
            return vcfc_gm::ST_E_ARG;
        table = built.data();
        table_bytes = bytes;
    }
    if (mode == 2 && !vcfc_reg::regions_validate(table, table_bytes)) return vcfc_gm::ST_E_ARG;
    const vcfc_gm::Query q{ref, ref_len, has_range, qstart, qend};
    vcfc_gm::Result R;
    uint64_t data_off = 0, S = 0;
    HostBuffers B;
    int st;
    if (mode == 2) {
        const uint8_t *d_table = nullptr;
        const vcfc_dec::MatchStep match = vcfc_reg::regions_step(table, table_bytes, &d_table);
        st = vcfc_gm::matrix_file(in, n, layout, &match, B, nullptr, R, &data_off, &S, rec_batch);
    } else {
        st = vcfc_gm::matrix_file(in, n, layout, mode ? &q : nullptr, B, nullptr, R, &data_off, &S, rec_batch);
    }
    if (st != vcfc_gm::ST_OK && st != vcfc_gm::ST_E_FORMAT) return st;
    *err_record = R.err_record;
    *n_rows = R.index.size();
    *n_samples = S;
    if (*n_rows > rows_cap) return 4;
    std::copy(R.index.begin(), R.index.end(), index);
    std::copy(R.rows.begin(), R.rows.end(), rows);
    if (layout == VCFC_MATRIX_BED && data_off && S) {
        std::vector<uint8_t> text;
        vcfc_gm::render_bed(R, text);
        if (text.size() > text_cap) return 4;
        memcpy(bed, text.data(), text.size());
        *bed_len = text.size();
        vcfc_gm::render_bim(in + data_off, R, text);
        if (text.size() > text_cap) return 4;
        memcpy(bim, text.data(), text.size());
        *bim_len = text.size();
        if (st == vcfc_gm::ST_OK) {
            vcfc_gm::render_fam(in, data_off, S, text);
            if (text.size() > text_cap) return 4;
            memcpy(fam, text.data(), text.size());
            *fam_len = text.size();
        }
    }
    return st;
}

// the device entry (the C ABI's vcfc_genotype_matrix_device, argument for
// argument) on records [rec[0], rec[n])
extern "C" int emu_matrix_device(const uint8_t *recs, const uint64_t *rec, const uint8_t *select, uint64_t n, uint64_t S,
                                 int layout, uint8_t *out, uint64_t out_cap, uint64_t row_stride, uint64_t *row_of,
                                 uint8_t *ws, uint64_t ws_bytes, uint64_t *err) {
    if (n >= (1ull << 32))   // (refused before rec[n] is looked at: nothing to copy)
        return vcfc_gm::matrix_device(recs, 0, rec, select, n, S, layout, out, out_cap, row_stride, row_of, ws, ws_bytes, err,
                                      nullptr);
    HostInput in(recs, n && rec ? rec[n] : 0);
    return vcfc_gm::matrix_device(recs ? in.p : nullptr, n && rec ? rec[n] : 0, rec, select, n, S, layout, out, out_cap,
                                  row_stride, row_of, ws, ws_bytes, err, nullptr);
}
