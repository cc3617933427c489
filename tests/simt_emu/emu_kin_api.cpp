// TEST INFRASTRUCTURE ONLY: C entry points that run the kinship kernels
// (csrc/vcfc_kin.hip) and their host driver (csrc/vcfc_kin_driver.h) on the
// fiber emulator, with host memory standing in for HBM.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vcfc_device.h"
#include "vcfc_kin_driver.h"
#include "vcfc_regions_driver.h"
#include "emu.h"
#include "host_buffers.h"

extern "C" uint64_t emu_kin_workspace_size(uint64_t n, uint64_t S) { return vcfc_kin_workspace_layout(n, S).total; }
extern "C" uint64_t emu_kin_tile_samples() { return VCFC_KIN_TILE_SAMPLES; }
extern "C" uint64_t emu_kin_chunk_words() { return VCFC_KIN_CHUNK_WORDS; }
extern "C" uint64_t emu_kin_plane_rows() { return VCFC_KIN_PLANE_ROWS; }
extern "C" uint64_t emu_kin_batch_need(uint64_t n, uint64_t S) { return vcfc_kin::batch_need(n, S); }
extern "C" uint64_t emu_kin_batch_records(uint64_t S, uint64_t ws_bound) { return vcfc_kin::batch_records(S, ws_bound); }

// kinship over a whole .vcfc (the C ABI's control flow): indices and the
// square up to rows_cap rows / tables_cap tables, and the text of the file
// entry where the header was accepted.  mode 0: every record, 1: one region,
// 2: a region table (`table` is region text: the table is built here).
extern "C" int emu_kin_file(const uint8_t *in, uint64_t n, int mode, const uint8_t *ref, uint64_t ref_len, int has_range,
                            uint64_t qstart, uint64_t qend, const uint8_t *table, uint64_t table_bytes, uint64_t ws_bound,
                            uint64_t *index, uint32_t *tables, uint64_t rows_cap, uint64_t tables_cap, uint64_t *n_rows,
                            uint64_t *n_samples, uint64_t *err_record, int has_min, double min_kinship, uint8_t *tsv,
                            uint64_t *tsv_len, uint64_t text_cap) {
    *n_rows = *n_samples = *tsv_len = 0;
    *err_record = ~0ull;
    std::vector<uint8_t> built;
    if (mode == 2) {
        uint64_t bytes = 0, n_regions = 0, bad_line = 0;
        built.resize(64 * table_bytes + 4096);
        if (vcfc_reg::regions_build(reinterpret_cast<const char *>(table), table_bytes, built.data(), built.size(), &bytes,
                                    &n_regions, &bad_line) != 0)
            return vcfc_kin::ST_E_ARG;
        table = built.data();
        table_bytes = bytes;
        if (!vcfc_reg::regions_validate(table, table_bytes)) return vcfc_kin::ST_E_ARG;
    }
    const vcfc_kin::Query q{ref, ref_len, has_range, qstart, qend};
    vcfc_kin::Result R;
    uint64_t data_off = 0, S = 0;
    HostBuffers B;
    int st;
    if (mode == 2) {
        const uint8_t *d_table = nullptr;
        const vcfc_dec::MatchStep match = vcfc_reg::regions_step(table, table_bytes, &d_table);
        st = vcfc_kin::kin_file(in, n, &match, B, nullptr, R, &data_off, &S, ws_bound);
    } else {
        st = vcfc_kin::kin_file(in, n, mode ? &q : nullptr, B, nullptr, R, &data_off, &S, ws_bound);
    }
    if (st != vcfc_kin::ST_OK && st != vcfc_kin::ST_E_FORMAT) return st;
    *err_record = R.err_record;
    *n_rows = R.index.size();
    *n_samples = S;
    if (*n_rows > rows_cap || R.tables.size() / 9 > tables_cap) return 4;
    std::copy(R.index.begin(), R.index.end(), index);
    std::copy(R.tables.begin(), R.tables.end(), tables);
    if (text_cap && data_off && S && !R.tables.empty()) {   // text_cap 0: the text is not asked for
        std::vector<uint8_t> text;
        vcfc_kin::render_tsv(in, data_off, S, R, has_min != 0, min_kinship, text);
        if (text.size() > text_cap) return 4;
        memcpy(tsv, text.data(), text.size());
        *tsv_len = text.size();
    }
    return st;
}

// the pair step (the C ABI's vcfc_kin_tables_device, argument for argument)
extern "C" int emu_kin_tables_device(const uint8_t *bed, uint64_t n_rows, uint64_t row_stride, uint64_t S, uint32_t *tables,
                                     uint64_t tables_cap, int accumulate, uint8_t *ws, uint64_t ws_bytes, uint64_t *err) {
    return vcfc_kin::tables_device(bed, n_rows, row_stride, S, tables, tables_cap, accumulate, ws, ws_bytes, err, nullptr);
}

// the composed call (the C ABI's vcfc_kin_records_device, argument for
// argument) on records [rec[0], rec[n])
extern "C" int emu_kin_records_device(const uint8_t *recs, const uint64_t *rec, const uint8_t *select, uint64_t n, uint64_t S,
                                      uint32_t *tables, uint64_t tables_cap, int accumulate, uint64_t *row_of, uint8_t *ws,
                                      uint64_t ws_bytes, uint64_t *err) {
    if (n >= (1ull << 32))   // (refused before rec[n] is looked at: nothing to copy)
        return vcfc_kin::records_device(recs, 0, rec, select, n, S, tables, tables_cap, accumulate, row_of, ws, ws_bytes, err,
                                        nullptr);
    HostInput in(recs, n && rec ? rec[n] : 0);
    return vcfc_kin::records_device(recs ? in.p : nullptr, n && rec ? rec[n] : 0, rec, select, n, S, tables, tables_cap,
                                    accumulate, row_of, ws, ws_bytes, err, nullptr);
}
