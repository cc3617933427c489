// TEST INFRASTRUCTURE ONLY: C entry points that run the ld-window kernels
// (csrc/vcfc_ld.hip) and their host driver (csrc/vcfc_ld_driver.h) on the
// fiber emulator, with host memory standing in for HBM.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vcfc_device.h"
#include "vcfc_ld_driver.h"
#include "vcfc_regions_driver.h"
#include "emu.h"
#include "host_buffers.h"

extern "C" uint64_t emu_ld_workspace_size(uint64_t n, uint64_t S, uint64_t) { return vcfc_ld_workspace_layout(n, S).total; }
extern "C" uint64_t emu_ld_tile_rows() { return VCFC_LD_TILE_ROWS; }
extern "C" uint64_t emu_ld_tile_partners() { return VCFC_LD_TILE_PARTNERS; }
extern "C" uint64_t emu_ld_chunk_samples() { return VCFC_LD_CHUNK_SAMPLES; }
extern "C" uint64_t emu_ld_matrix_lds_samples() { return vcfc_matrix_tile_samples(VCFC_MATRIX_BED); }

// ld-window over a whole .vcfc (the C ABI's control flow): indices and the
// band up to rows_cap rows / pairs_cap slots, and the text of the file entry
// where the header was accepted.  mode 0: every record, 1: one region, 2: a
// region table (`table` is region text: the table is built here).
extern "C" int emu_ld_file(const uint8_t *in, uint64_t n, uint64_t W, int mode, const uint8_t *ref, uint64_t ref_len,
                           int has_range, uint64_t qstart, uint64_t qend, const uint8_t *table, uint64_t table_bytes,
                           uint64_t band_bound, uint64_t *index, uint32_t *tables, uint64_t rows_cap, uint64_t pairs_cap,
                           uint64_t *n_rows, uint64_t *err_record, double min_r2, uint8_t *tsv, uint64_t *tsv_len,
                           uint64_t text_cap) {
    *n_rows = *tsv_len = 0;
    *err_record = ~0ull;
    std::vector<uint8_t> built;
    if (mode == 2) {
        uint64_t bytes = 0, n_regions = 0, bad_line = 0;
        built.resize(64 * table_bytes + 4096);
        if (vcfc_reg::regions_build(reinterpret_cast<const char *>(table), table_bytes, built.data(), built.size(), &bytes,
                                    &n_regions, &bad_line) != 0)
            return vcfc_ld::ST_E_ARG;
        table = built.data();
        table_bytes = bytes;
        if (!vcfc_reg::regions_validate(table, table_bytes)) return vcfc_ld::ST_E_ARG;
    }
    const vcfc_ld::Query q{ref, ref_len, has_range, qstart, qend};
    vcfc_ld::Result R;
    uint64_t data_off = 0, S = 0;
    HostBuffers B;
    int st;
    if (mode == 2) {
        const uint8_t *d_table = nullptr;
        const vcfc_dec::MatchStep match = vcfc_reg::regions_step(table, table_bytes, &d_table);
        st = vcfc_ld::window_file(in, n, W, &match, B, nullptr, R, &data_off, &S, band_bound);
    } else {
        st = vcfc_ld::window_file(in, n, W, mode ? &q : nullptr, B, nullptr, R, &data_off, &S, band_bound);
    }
    if (st != vcfc_ld::ST_OK && st != vcfc_ld::ST_E_FORMAT) return st;
    *err_record = R.err_record;
    *n_rows = R.index.size();
    if (*n_rows > rows_cap || R.tables.size() / 9 > pairs_cap) return 4;
    std::copy(R.index.begin(), R.index.end(), index);
    std::copy(R.tables.begin(), R.tables.end(), tables);
    if (data_off && S) {
        std::vector<uint8_t> text;
        vcfc_ld::render_tsv(in + data_off, R, W, min_r2, text);
        if (text.size() > text_cap) return 4;
        memcpy(tsv, text.data(), text.size());
        *tsv_len = text.size();
    }
    return st;
}

// the pair step (the C ABI's vcfc_ld_tables_device, argument for argument)
extern "C" int emu_ld_tables_device(const uint8_t *bed, uint64_t n_rows, uint64_t row_stride, uint64_t S, uint64_t W,
                                    uint32_t *tables, uint64_t pairs_cap, uint8_t *ws, uint64_t ws_bytes, uint64_t *err) {
    return vcfc_ld::tables_device(bed, n_rows, row_stride, S, W, tables, pairs_cap, ws, ws_bytes, err, nullptr);
}

// the composed call (the C ABI's vcfc_ld_window_device, argument for
// argument) on records [rec[0], rec[n])
extern "C" int emu_ld_window_device(const uint8_t *recs, const uint64_t *rec, const uint8_t *select, uint64_t n, uint64_t S,
                                    uint64_t W, uint32_t *tables, uint64_t pairs_cap, uint64_t *row_of, uint8_t *ws,
                                    uint64_t ws_bytes, uint64_t *err) {
    if (n >= (1ull << 32))   // (refused before rec[n] is looked at: nothing to copy)
        return vcfc_ld::window_device(recs, 0, rec, select, n, S, W, tables, pairs_cap, row_of, ws, ws_bytes, err, nullptr);
    HostInput in(recs, n && rec ? rec[n] : 0);
    return vcfc_ld::window_device(recs ? in.p : nullptr, n && rec ? rec[n] : 0, rec, select, n, S, W, tables, pairs_cap,
                                  row_of, ws, ws_bytes, err, nullptr);
}
