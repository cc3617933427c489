// vcfc_device.h -- device-side launch interface shared by the C-ABI
// (vcfc_api.cpp) and the kernels (vcfc_encode.hip).  Plain pointers only.
#pragma once
// The kernels' diagnostic switches make libvcfc.so write WRONG .vcfc bytes
// (they remove steps to price them: profiles/r04/ab/*bisect*).  They exist for
// the A/B builds under build_ab/ only, which must also define
// VCFC_DIAG_BUILD; a product build with any of them is refused here (and by
// the Makefile, tests/test_capi.py::test_diag_switches_refused).
#if (defined(VCFC_DIAG_NOSTORE) || defined(VCFC_DIAG_NOSTEP) || defined(VCFC_DIAG_CLEAN_SKIP) || \
     defined(VCFC_VAR_SIZE_ONLY) || defined(VCFC_DIAG_DEC_NOSCAN) || defined(VCFC_DIAG_NOESCEMIT) || \
     defined(VCFC_DIAG_NODIRECT) || defined(VCFC_DIAG_HOP_TWICE)) && \
    !defined(VCFC_DIAG_BUILD)
#error "VCFC_DIAG_* / VCFC_VAR_SIZE_ONLY produce wrong output: diagnostic builds only (define VCFC_DIAG_BUILD)"
#endif
#include <stddef.h>
// deferred records on (1) or off (0) by default (A/B builds set 0)
#ifndef VCFC_DEFER_DEFAULT
#define VCFC_DEFER_DEFAULT 1
#endif
#include <stdint.h>
#include <hip/hip_runtime.h>

// status codes (identical to include/vcfc.h)
#define VCFCD_OK 0
#define VCFCD_E_LT8COLS 1
#define VCFCD_E_8COLS 2
#define VCFCD_E_NOSPACE 4
// a row holding a '\n' byte, seen only when VcfcEncodeArgs::nl_check is set:
// the hop line index (vcfc_line_index with S_hint) mispredicted a line end
#define VCFCD_E_NEWLINE 9
// a deferred record came out another size than it was sized (cannot happen;
// reported as VCFC_E_HIP, a device failure)
#define VCFCD_E_INTERNAL 6
// a line longer than VCFCD_MAX_LINE (include/vcfc.h VCFC_E_TOOLONG): records
// stay below 2^30 bytes, the LEN header's range, so that every rec_size flag
// below (VCFCD_RETRY_GT, VCFCD_DEFER: the top two bits) is free of sizes
#define VCFCD_E_TOOLONG 10
#define VCFCD_MAX_LINE ((1u << 29) - 64u)

// error word: min over failing rows of (row << 8 | code); ~0 = no error
#define VCFCD_NO_ERROR (~0ull)
// rec_size value of a row the fast kernel leaves to k_encode_var
#define VCFCD_RETRY 0xFFFFFFFFu
// ... or, when k_encode_fast parsed a clean prefix inside the line's first
// 1 KiB and only the genotype tokens were of another shape, VCFCD_RETRY_GT |
// the first sample's offset (< VCFCD_GT0_NONE): k_encode_var skips the parse
#define VCFCD_RETRY_GT 0xC0000000u
#define VCFCD_GT0_NONE 0x3FFFFFFFu
// ... with this bit when the row starts with escapes -- its first token is 5
// bytes or longer (GT:DP:GQ and the like), or every token of its first 2 KiB
// genotype chunk is a 3-byte escape (unphased "0/1", "./."): with deferred
// records k_encode_var predicts its record without reading it (the offset
// itself is < 1 KiB)
#define VCFCD_GT0_LONG 0x20000000u
// rec_size flag of a deferred row: k_encode_var only sized it (every chunk an
// escape chunk), k_encode_defer writes its record straight to out after the
// size scan (the size is the low 31 bits)
#define VCFCD_DEFER 0x80000000u

// Alignment: buf, the lines in it and out may start at any byte.  The
// kernels address them with 16-byte loads and stores at the base's own
// alignment (k_nl_scan reads a chunk from d_in + pos, k_nl_hop a line's
// windows from any byte of it, k_compact_out stores
// 16-B blocks at out + 16k, out = d_out + header bytes in compress_device);
// gfx950 global and buffer memory instructions take unaligned addresses (ROCm
// runs the GPU with SH_MEM_CONFIG's unaligned mode), an unaligned base only
// costs the split accesses.  tests/test_gpu_ingest.py and test_kernel_emu.py
// run unaligned bases and chunk starts (all 16 alignments of the buffer).
struct VcfcEncodeArgs {
    // input: concatenated VCF data lines (device memory)
    const uint8_t *buf;
    const uint64_t *line_off;  // byte offset of line i in buf
    const uint32_t *line_len;  // length of line i, without '\n'
    uint64_t n;                // rows
    uint64_t line_bytes_hint;  // sum of the line lengths (<= the workspace's total_line_bytes): picks the compaction shape
    // output
    uint8_t *out;              // records, concatenated in row order
    uint64_t out_cap;
    uint64_t *rec_off;         // n + 1 exclusive offsets; rec_off[n] = total
    // workspace (see vcfc_encode_workspace_layout)
    uint64_t *slot_off;        // n + 1
    uint32_t *rec_size;        // n
    uint64_t *partials;        // scan partials
    uint64_t *err;             // 1 word
    uint32_t *retry_count;     // rows that took the general path (emulator builds only, diag hooks)
    uint32_t *defer_count;     // deferred rows (VCFCD_DEFER), zeroed per encode with lb
    uint32_t *defer_list;      // their row indices (any order), n entries
    // predicted deferred records (k_encode_var sizes an all-escape row from
    // its first chunk and the token count two earlier rows agreed on;
    // k_encode_defer's first pass checks every record against its size):
    uint32_t *mispredict;      // nonzero: some record's size was wrong -- the size scan, compaction and
                               // deferred writes run again on the exact sizes (gated launches)
    uint32_t *defer_fallback;  // deferred rows not written straight to out: the general path after all, a '\n', the cap
    uint64_t *nospace;         // the first size scan's out_cap report (row << 8 | VCFCD_E_NOSPACE),
                               // merged into err unless the scan runs again
    uint8_t *lb;               // look-back scan state (tickets, tile flags; zeroed per encode)
    uint32_t *tile_first;      // per 4 KiB output tile: the row holding its first byte (compaction)
    uint8_t *prim;             // per-row primary staging: record bytes [0, prim_bytes) at prim + prim_bytes * row
    uint8_t *slots;            // per-row overflow slots: record bytes [prim_bytes, ...) at slots + slot_off[row]
    uint32_t prim_bytes;       // vcfc_prim_bytes of the workspace layout
    uint64_t slots_cap;
    uint64_t *dbg;             // diagnostic builds only (tools/diag hooks); else null
    // rows from the hop line index: a row holding a '\n' fails with
    // VCFCD_E_NEWLINE (k_encode_var scans the rows k_encode_fast hands back;
    // k_encode_fast accepts none)
    uint32_t nl_check = 0;
    // deferred records (k_encode_var sizes the rows whose first genotype
    // chunk is all escapes and that span more than one chunk, k_encode_defer
    // writes them to out after the size scan): on by
    // default since round 5 -- the choice is made per row by the kernel from
    // the row's own bytes, and a batch without such rows pays one empty
    // launch; vcfc_ctx_set_deferred_records(ctx, 0) turns it off
    uint32_t defer_records = VCFC_DEFER_DEFAULT;
};

// Record staging: the first prim_bytes bytes of every record go to a dense
// per-row array (the compaction then reads most records from consecutive
// kilobytes), the rest (records of rare escape-heavy rows) to a per-row
// overflow slot sized for the worst case.  2 KiB for batches of long lines
// (mean >= 4 KiB: records of 1-2 KiB, e.g. the random_vcf law's ~1.28 KB at
// 2504 samples, stay in one region; k_compact -14 % on law 0 and -9 % on
// law 1 in an A/B, 4 KiB slower again, profiles/r03/ab/ab_prim*.txt), else
// 1 KiB (the region costs prim_bytes per row whatever the line length).
// A multiple of the 1 KiB flush burst, so no burst straddles the regions.
__host__ __device__ inline uint32_t vcfc_prim_bytes(uint64_t n, uint64_t total_line_bytes) {
    return n && total_line_bytes / n >= 4096 ? 2048u : 1024u;
}

struct VcfcWorkspaceLayout {
    uint64_t slot_off, rec_size, partials, err, lb, lb_bytes, retry_count, defer_count, mispredict, defer_fallback,
        nospace, defer_list, tile_first, prim, slots, dbg, total;
    uint32_t prim_bytes;
};

// Bytes of per-row staging for a line of `len` bytes: covers the worst-case
// record (8 + len + (len+1)/2 + 2) plus the 16-byte flush granule.
__host__ __device__ inline uint64_t vcfc_slot_bytes(uint32_t len) {
    return ((uint64_t)len + (len >> 1) + 48 + 15) & ~15ull;
}

// Upper bound of the records of n rows whose line bytes sum to total
// (include/vcfc.h vcfc_encode_bound).
__host__ __device__ inline uint64_t vcfc_record_bound(uint64_t n, uint64_t total) {
    return total + total / 2 + 16 * n + 16;
}

// Workspace layout for n rows whose line lengths sum to <= total_line_bytes.
VcfcWorkspaceLayout vcfc_encode_workspace_layout(uint64_t n, uint64_t total_line_bytes);

// Point a's workspace arrays into ws (err is the caller's).
inline void vcfc_encode_args_workspace(VcfcEncodeArgs &a, uint8_t *ws, const VcfcWorkspaceLayout &L) {
    a.slot_off = reinterpret_cast<uint64_t *>(ws + L.slot_off);
    a.rec_size = reinterpret_cast<uint32_t *>(ws + L.rec_size);
    a.partials = reinterpret_cast<uint64_t *>(ws + L.partials);
    a.retry_count = reinterpret_cast<uint32_t *>(ws + L.retry_count);
    a.defer_count = reinterpret_cast<uint32_t *>(ws + L.defer_count);
    a.defer_list = reinterpret_cast<uint32_t *>(ws + L.defer_list);
    a.mispredict = reinterpret_cast<uint32_t *>(ws + L.mispredict);
    a.defer_fallback = reinterpret_cast<uint32_t *>(ws + L.defer_fallback);
    a.nospace = reinterpret_cast<uint64_t *>(ws + L.nospace);
    a.lb = ws + L.lb;
    a.tile_first = reinterpret_cast<uint32_t *>(ws + L.tile_first);
    a.prim = ws + L.prim;
    a.prim_bytes = L.prim_bytes;
    a.slots = ws + L.slots;
    a.slots_cap = L.dbg - L.slots;
    a.dbg = L.dbg < L.total ? reinterpret_cast<uint64_t *>(ws + L.dbg) : nullptr;
}

// Rows the last encode on this workspace deferred (the device word behind
// VcfcEncodeArgs::defer_count; read by the caller after the stream is done).
inline uint64_t vcfc_defer_count_offset(const VcfcWorkspaceLayout &L) { return L.defer_count; }
// ... of which this many were written by the general path after all (a
// predicted all-escape row whose later chunks had another shape)
inline uint64_t vcfc_defer_fallback_offset(const VcfcWorkspaceLayout &L) { return L.defer_fallback; }

// Enqueue the whole encode on `stream` (no host synchronisation, capturable).
// If `ev` is non-null, ev[0..5] are recorded before the slot scan, after it,
// after k_encode (fast + variable-token kernels), after the size scan, after
// k_compact and after k_encode_defer.
hipError_t vcfc_encode_device(const VcfcEncodeArgs &a, hipStream_t stream, hipEvent_t *ev = nullptr);

// ---------------------------------------------------------------------------
// Decoder (vcfc_decode.hip).  Records of one batch, located by LEN hops.
struct VcfcDecodeArgs {
    const uint8_t *in;          // data section bytes (device)
    uint64_t n_bytes;           // bytes available from `in` (the byte-serial parse may read past a record)
    const uint64_t *rec_start;  // n + 1 record offsets into `in` (rec_start[n] = end of the hopped range)
    const uint8_t *select;      // nullptr, or per record: 0 = skip it (no line; the range query's non-matches)
    uint64_t n;                 // records
    uint64_t S;                 // samples declared by the header line
    uint8_t *out;               // decoded lines, concatenated
    uint64_t out_cap;
    uint64_t *line_off;         // n + 1 exclusive offsets of the lines in `out`
    // workspace (vcfc_decode_workspace_layout)
    uint32_t *st;               // per-record plan status
    uint32_t *line_size;        // per-record line bytes
    uint64_t *end;              // byte-serial parse end (queued records)
    uint32_t *seq_list;         // records queued for the byte-serial path
    uint32_t *seq_count;
    uint64_t *err;              // min over records of (i << 8 | code): 2 = parse ends off the hop, 3 = reference error,
                                // 4 = light plan was wrong (rerun exactly), 0xFF = out_cap short
    uint64_t *partials;         // scan partials
};

struct VcfcDecodeLayout {
    uint64_t st, line_size, end, seq_list, seq_count, err, partials, total;
};

VcfcDecodeLayout vcfc_decode_workspace_layout(uint64_t n);
// plan: statuses, sizes, line offsets (no host synchronisation).  exact =
// false scans only headers and REQ and assumes the sample sections are
// simple; k_dec_write then reports (i << 8 | 4) in err for a record where
// that was wrong, and the batch must be planned again with exact = true.
hipError_t vcfc_decode_plan(const VcfcDecodeArgs &a, bool exact, hipStream_t s);
// write lines [first, last) at a.out + line_off[i] (their plan status must not be an error)
hipError_t vcfc_decode_write(const VcfcDecodeArgs &a, uint64_t first, uint64_t last, hipStream_t s);
// one-lane byte-serial decode of in[p, n), at most max_lines lines: out ==
// nullptr counts; st[0..3] = {0 max_lines reached | 1 clean end | 2 reference
// error, bytes, lines, parse end}
hipError_t vcfc_decode_stream(const uint8_t *in, uint64_t n, uint64_t p, uint64_t S, uint64_t max_lines,
                              uint8_t *out, uint64_t *st, hipStream_t s);
// per-record 64-bit digests of records[rec_off[i], rec_off[i + 1]) (vcfc_check.hip)
hipError_t vcfc_record_hash(const uint8_t *recs, const uint64_t *rec_off, uint64_t n, uint64_t *out, hipStream_t s);
// exclusive u32 -> u64 scan with out[n] = total (shared with the encoder)
hipError_t vcfc_scan_u32(const uint32_t *in, uint64_t n, uint64_t *partials, uint64_t *out, hipStream_t s);
// The same over line kinds (bit 0: data line, bit 1: '#' line): out[i] =
// data lines before i | '#' lines before i << 32 (line index phase 2).
hipError_t vcfc_scan_kinds(const uint32_t *in, uint64_t n, uint64_t *partials, uint64_t *out, hipStream_t s);

// ---------------------------------------------------------------------------
// Sample-subset decoder (vcfc_subset.hip): REQ and K chosen
// sample columns of every record.  A record that is not regular (DESIGN.md
// §4i) gets no line and is reported in err.
struct VcfcSubsetArgs {
    const uint8_t *in;          // data section bytes (device)
    uint64_t n_bytes;
    const uint64_t *rec_start;  // n + 1 record offsets into `in`
    const uint8_t *select;      // nullptr, or per record: 0 = skip it (no line, not checked)
    uint64_t n;                 // records
    uint64_t S;                 // samples declared by the header line (1 <= S < 2^31)
    const uint32_t *csort;      // the K chosen columns, ascending (distinct, < S)
    const uint32_t *rank;       // rank[k]: output slot of column csort[k]
    uint32_t K;                 // 1 <= K <= S
    uint8_t *out;               // lines, concatenated
    uint64_t out_cap;
    uint64_t *line_off;         // n + 1 exclusive offsets of the lines in `out`
    // workspace (vcfc_subset_workspace_layout)
    uint32_t *st;               // per-record plan status
    uint32_t *line_size;        // per-record line bytes
    uint32_t *seq_list;         // records left to the byte-serial path
    uint32_t *seq_count;
    uint64_t *err;              // min over records of (i << 8 | code): 3 = not regular, 0xFF = out_cap short
    uint64_t *partials;         // scan partials
    uint32_t *seq_scratch;      // VCFC_SUBSET_SEQ_LANES * K words: token offsets of the byte-serial writer
};
// lanes of the byte-serial writer (each owns K words of seq_scratch)
#define VCFC_SUBSET_SEQ_LANES 1024u

struct VcfcSubsetLayout {
    uint64_t st, line_size, seq_list, seq_count, err, partials, csort, rank, seq_scratch, total;
};
VcfcSubsetLayout vcfc_subset_workspace_layout(uint64_t n, uint64_t K);
// Point a's workspace arrays into ws (err, csort and rank included).
inline void vcfc_subset_args_workspace(VcfcSubsetArgs &a, uint8_t *ws, const VcfcSubsetLayout &L) {
    a.st = reinterpret_cast<uint32_t *>(ws + L.st);
    a.line_size = reinterpret_cast<uint32_t *>(ws + L.line_size);
    a.seq_list = reinterpret_cast<uint32_t *>(ws + L.seq_list);
    a.seq_count = reinterpret_cast<uint32_t *>(ws + L.seq_count);
    a.err = reinterpret_cast<uint64_t *>(ws + L.err);
    a.partials = reinterpret_cast<uint64_t *>(ws + L.partials);
    a.csort = reinterpret_cast<uint32_t *>(ws + L.csort);
    a.rank = reinterpret_cast<uint32_t *>(ws + L.rank);
    a.seq_scratch = reinterpret_cast<uint32_t *>(ws + L.seq_scratch);
}
// exact plan: statuses, line sizes, line offsets, err (no host synchronisation)
hipError_t vcfc_subset_plan(const VcfcSubsetArgs &a, hipStream_t s);
// write lines [first, last) at a.out + line_off[i] (after vcfc_subset_plan)
hipError_t vcfc_subset_write(const VcfcSubsetArgs &a, uint64_t first, uint64_t last, hipStream_t s);

// ---------------------------------------------------------------------------
// Extract (vcfc_extract.hip): REQ and K chosen sample columns of
// every record, as a .vcfc record again.  The subset decoder's argument block
// and workspace arrays, read as: out = records, line_size / line_off = record
// sizes / offsets, seq_scratch = 2 * VCFC_EXTRACT_SEQ_LANES * K words, err
// codes 3 = not regular, 5 = regular but not re-encodable, 0xFF = out_cap short.
typedef VcfcSubsetArgs VcfcExtractArgs;
#define VCFC_EXTRACT_SEQ_LANES 1024u
// chosen columns the wave path's LDS tile holds; above it every record takes the byte-serial path
#define VCFC_EXTRACT_TILE 4096u
VcfcSubsetLayout vcfc_extract_workspace_layout(uint64_t n, uint64_t K);
// exact plan: statuses, record sizes, record offsets, err (no host synchronisation)
hipError_t vcfc_extract_plan(const VcfcExtractArgs &a, hipStream_t s);
// write records [first, last) at a.out + line_off[i] (after vcfc_extract_plan)
hipError_t vcfc_extract_write(const VcfcExtractArgs &a, uint64_t first, uint64_t last, hipStream_t s);

// ---------------------------------------------------------------------------
// Genotype counts (vcfc_counts.hip): per record a row of eight
// counters, per sample five, both taken from the run-length code without
// decoding it.  A record that is not regular is reported in
// err.
struct VcfcCountsArgs {
    const uint8_t *in;          // data section bytes (device)
    uint64_t n_bytes;
    const uint64_t *rec_start;  // n + 1 record offsets into `in`
    const uint8_t *select;      // nullptr, or per record: 0 = skip it (zero row, not counted, not checked)
    uint64_t n;                 // records (< 2^32)
    uint64_t S;                 // samples declared by the header line (1 <= S < 2^30)
    uint32_t *variant;          // nullptr, or 8 n words: n00 n01 n10 n11 n_other AN AC1 AC_other per record
    uint64_t *sample;           // nullptr, or 5 S words, ADDED to: c00 c01 c10 c11 c_other per sample
    // workspace (vcfc_counts_workspace_layout)
    uint64_t *hist;             // 4 S words, class-major: this call's c01 c10 c11 c_other
    uint64_t *counted;          // records counted by this call
    uint32_t *seq_list;         // records left to the byte-serial path
    uint32_t *seq_count;
    uint64_t *err;              // min over records of (i << 8 | 3): not regular
};
// samples whose 4 x uint32 counters fit the LDS tile k_cnt_scan is built with
// (16 S bytes <= 40 KiB); above it the histogram takes global atomics
#define VCFC_COUNTS_LDS_SAMPLES 2560u

struct VcfcCountsLayout {
    uint64_t hist, counted, seq_list, seq_count, err, total;
};
VcfcCountsLayout vcfc_counts_workspace_layout(uint64_t n, uint64_t S);
// Point a's workspace arrays into ws (err included).
inline void vcfc_counts_args_workspace(VcfcCountsArgs &a, uint8_t *ws, const VcfcCountsLayout &L) {
    a.hist = reinterpret_cast<uint64_t *>(ws + L.hist);
    a.counted = reinterpret_cast<uint64_t *>(ws + L.counted);
    a.seq_list = reinterpret_cast<uint32_t *>(ws + L.seq_list);
    a.seq_count = reinterpret_cast<uint32_t *>(ws + L.seq_count);
    a.err = reinterpret_cast<uint64_t *>(ws + L.err);
}
// one scan of every (selected) record: rows, the sample table, err (no host
// synchronisation)
hipError_t vcfc_counts_run(const VcfcCountsArgs &a, hipStream_t s);
// records one pass of the scan's resident grid covers on the current device
// (a longer call goes round the grid again); 0 where the device cannot be asked
uint64_t vcfc_counts_scan_trip(uint64_t S, bool with_sample_table);

// ---------------------------------------------------------------------------
// Genotype matrix (vcfc_matrix.hip): per (selected) record one
// row of the variants x samples matrix, written out of the run-length code:
// int8 dosage, the two int8 haplotype planes interleaved, or PLINK 1 .bed
// 2-bit codes.  A record that is not regular is reported in
// err.
#define VCFC_MATRIX_DOSAGE 0
#define VCFC_MATRIX_HAP 1
#define VCFC_MATRIX_BED 2
struct VcfcMatrixArgs {
    const uint8_t *in;          // data section bytes (device)
    uint64_t n_bytes;
    const uint64_t *rec_start;  // n + 1 record offsets into `in`
    const uint8_t *select;      // nullptr, or per record: 0 = no row (not checked)
    uint64_t n;                 // records (< 2^32)
    uint64_t S;                 // samples declared by the header line (1 <= S < 2^30)
    int layout;                 // VCFC_MATRIX_*
    uint8_t *out;               // row r at out + r * row_stride; nothing at or past out + out_cap
    uint64_t out_cap, row_stride;
    uint64_t *row_of;           // n + 1 words: row_of[i] = selected records before i; row_of[n] = rows
    // workspace (vcfc_matrix_workspace_layout)
    uint32_t *flag32;           // the select flags as words (the scan's input)
    uint64_t *partials;         // scan partials
    uint32_t *seq_list;         // records left to the byte-serial path
    uint32_t *seq_count;
    uint64_t *err;              // min over records of (i << 8 | 3): not regular, (i << 8 | 0xFF): row past out_cap
};
// bytes of a row (0: unknown layout); constexpr: host and device
constexpr uint64_t vcfc_matrix_row_size(int layout, uint64_t S) {
    return layout == VCFC_MATRIX_DOSAGE ? S : layout == VCFC_MATRIX_HAP ? 2 * S : layout == VCFC_MATRIX_BED ? (S + 3) / 4 : 0;
}
// samples whose row fits the per-wave LDS tile k_gm_scan is built with
// (5120 row bytes and their alignment slack; .bed: 4096 one-byte codes and
// the packed row); above it the byte-serial kernel writes every row
#define VCFC_MATRIX_TILE_BYTES 5136u
constexpr uint64_t vcfc_matrix_tile_samples(int layout) {
    return layout == VCFC_MATRIX_DOSAGE ? 5120u : layout == VCFC_MATRIX_HAP ? 2560u : layout == VCFC_MATRIX_BED ? 4096u : 0u;
}
struct VcfcMatrixLayout {
    uint64_t flag32, partials, seq_list, seq_count, total;
};
VcfcMatrixLayout vcfc_matrix_workspace_layout(uint64_t n);
inline void vcfc_matrix_args_workspace(VcfcMatrixArgs &a, uint8_t *ws, const VcfcMatrixLayout &L) {
    a.flag32 = reinterpret_cast<uint32_t *>(ws + L.flag32);
    a.partials = reinterpret_cast<uint64_t *>(ws + L.partials);
    a.seq_list = reinterpret_cast<uint32_t *>(ws + L.seq_list);
    a.seq_count = reinterpret_cast<uint32_t *>(ws + L.seq_count);
}
// row_of, then one pass over every (selected) record: its row, err (no host
// synchronisation)
hipError_t vcfc_matrix_run(const VcfcMatrixArgs &a, hipStream_t s);
// records one pass of the scan's resident grid covers on the current device
// (S <= vcfc_matrix_tile_samples(layout)); 0 for an unknown layout or where
// the device cannot be asked
uint64_t vcfc_matrix_scan_trip(int layout);

// ---------------------------------------------------------------------------
// LD window (vcfc_ld.hip): the 3 x 3 genotype table of every
// pair of .bed rows (i, i + k), k = 1..W, by AND + population count over three
// bit planes a row (H: g = 1, B: g = 2, V: called; 32 samples a word).
#define VCFC_LD_TILE_ROWS 16u        // rows i one block of k_ld_pairs owns
#define VCFC_LD_TILE_PARTNERS 64u    // partners k one block covers (gridDim.y tiles of them)
#define VCFC_LD_CHUNK_SAMPLES 512u   // samples of every staged row in LDS at a time
struct VcfcLdArgs {
    const uint8_t *bed;         // .bed rows, row r at bed + r * row_stride (any alignment)
    uint64_t row_stride;
    uint64_t n;                 // rows at most (the grids are sized by it)
    const uint64_t *rows_dev;   // device word that holds the row count (<= n), or nullptr: n rows
    const uint8_t *select;      // with rows_dev: the records' flags (or nullptr) and row_of, for the
    const uint64_t *row_of;     //   record a short pairs_cap is reported at
    uint64_t S, W;
    uint32_t *tables;           // slot i * W + k - 1: nine words; nothing at or past slot pairs_cap
    uint64_t pairs_cap;
    uint64_t *err;
    bool own_err;               // the call resets err itself (no matrix call before it)
    // workspace (vcfc_ld_workspace_layout)
    uint64_t *state;            // [0] rows, [1] rows whose W slots all lie inside pairs_cap
    uint32_t *planes;           // row r, plane p at planes + (3 r + p) * plane_words
    uint64_t plane_words;       // a multiple of 4 (16 bytes)
};
struct VcfcLdLayout {
    uint64_t state, planes, bed, bed_stride, plane_words, matrix, total;
};
VcfcLdLayout vcfc_ld_workspace_layout(uint64_t n, uint64_t S);
// reset, planes, pairs: enqueued on s, no host synchronisation
hipError_t vcfc_ld_run(const VcfcLdArgs &a, hipStream_t s);

// ---------------------------------------------------------------------------
// Kinship (vcfc_kin.hip): the 3 x 3 genotype table of every
// pair of samples over the .bed rows, by AND + population count over three
// sample-major bit planes (H: g = 1, B: g = 2, V: called; 32 variants a word).
#define VCFC_KIN_TILE_SAMPLES 32u    // a block of k_kin_pairs owns a tile of 32 x 32 sample pairs
#define VCFC_KIN_CHUNK_WORDS 16u     // variant words of every staged sample in LDS at a time
#define VCFC_KIN_PLANE_ROWS 256u     // variant rows a block of k_kin_planes covers (32 bytes a sample and plane)
struct VcfcKinArgs {
    const uint8_t *bed;         // .bed rows, row r at bed + r * row_stride (any alignment)
    uint64_t row_stride;
    uint64_t n;                 // rows at most (the workspace and the grids are sized by it)
    const uint64_t *row_of;     // nullptr: n rows; else the matrix call's row_of (n + 1 words): row_of[n] rows,
                                //   cut to row_of[k] where err holds (k << 8 | 3)
    uint64_t S;
    uint32_t *tables;           // table (i, j) at tables + (i * S + j) * 9
    int accumulate;             // != 0: add to what tables holds
    uint64_t *err;
    bool own_err;               // the call resets err itself (no matrix call before it)
    // workspace (vcfc_kin_workspace_layout)
    uint64_t *state;            // [0] the rows that are counted
    uint32_t *planes;           // sample s, plane p at planes + (3 s + p) * row_words
    uint64_t row_words;         // a multiple of 4 (16 bytes); every bit at or past the row count is 0
};
struct VcfcKinLayout {
    uint64_t state, planes, bed, bed_stride, row_words, matrix, total;
};
VcfcKinLayout vcfc_kin_workspace_layout(uint64_t n, uint64_t S);
// reset, planes, pairs: enqueued on s, no host synchronisation
hipError_t vcfc_kin_run(const VcfcKinArgs &a, hipStream_t s);

// ---------------------------------------------------------------------------
// Range query (vcfc_decode.hip; reference query_compressed_file,
// src/main.cpp:3777-3929).  `ref` is device memory.
struct VcfcQuery {
    const uint8_t *ref;   // reference name; ref_len == 0 matches every name
    uint32_t ref_len;
    uint32_t has_range;   // 0: name only
    uint64_t start, end;  // inclusive position range
};
// one lane per record [rec_start[i], rec_start[i + 1]): flag[i] = 1 if the
// record matches; err = min over records of (i << 8 | code), code 2 = its
// POS does not parse (the reference throws), 3 = its CHROM or POS field runs
// past the record (the reference's walk leaves the LEN hops: continue with
// vcfc_query_stream from record i)
hipError_t vcfc_query_match(const uint8_t *in, const uint64_t *rec_start, uint64_t n, const VcfcQuery &q,
                            uint8_t *flag, uint64_t *err, hipStream_t s);
// one-lane byte-serial query of in[p, n) (st as vcfc_decode_stream)
hipError_t vcfc_query_stream(const uint8_t *in, uint64_t n, uint64_t p, uint64_t S, const VcfcQuery &q, uint8_t *out,
                             uint64_t *st, hipStream_t s);

// ---------------------------------------------------------------------------
// Region-list match (vcfc_regions.hip).  The table is one
// position-independent blob, built and validated on the host
// (vcfc_regions_driver.h), little-endian, offsets from its first byte:
//   VcfcRegionsHeader
//   VcfcRegionName[n_names]   sorted by (len, bytes); the wildcard "" is first
//   uint64 starts[n_intervals], uint64 ends[n_intervals]   (8-byte aligned)
//   the names' bytes
// A name's intervals [iv_first, iv_first + iv_count) are sorted by start and
// disjoint, so the last start <= POS decides a record.
#define VCFC_REGIONS_MAGIC 0x47524356u   // "VCRG"
#define VCFC_REGIONS_VERSION 1u
struct VcfcRegionsHeader {
    uint32_t magic, version;
    uint32_t n_names, n_intervals;
    uint32_t off_names, off_starts, off_ends, off_bytes;
    uint32_t total_bytes;   // the blob's size (< 4 GiB)
    uint32_t n_bytes;       // bytes of all names
    uint32_t pad[2];
};
struct VcfcRegionName {
    uint32_t byte_off;      // from off_bytes
    uint32_t len;
    uint32_t iv_first, iv_count;
};
// one lane per record, as vcfc_query_match (same flags' meaning, same err
// word): flag[i] = 1 if the record matches a region of the validated table
// at `table` (device memory)
hipError_t vcfc_regions_match(const uint8_t *in, const uint64_t *rec_start, uint64_t n, const uint8_t *table,
                              uint8_t *flag, uint64_t *err, hipStream_t s);

// ---------------------------------------------------------------------------
// Line index of an input chunk (vcfc_ingest.hip; reference compress()'s
// getline loop, src/compress.cpp:218-238).
struct VcfcLineIndex {
    uint64_t *line_off;     // data line j: chunk offset, length, 0-based line number in the chunk
    uint32_t *line_len;
    uint32_t *line_no;
    uint64_t *pass_off;     // '#' line q: chunk offset, length, line number, data lines before it
    uint32_t *pass_len;
    uint32_t *pass_no;
    uint64_t *pass_before;
    uint64_t *counts;       // {lines, data lines, pass lines, a line of >= 4 GiB}
};
struct VcfcLineIndexLayout {
    uint64_t seg_cnt, seg_base, slot, wstart, partials1, total1;     // phase 1 workspace
    uint64_t nl, kind, rank, partials2, total2;   // phase 2 workspace
};
VcfcLineIndexLayout vcfc_line_index_layout(uint64_t chunk_bytes, uint64_t n_lines);
// phase 1: '\n' count of buf[0, n) (last byte '\n'); counts[0] = lines.
// S_hint (the header's sample count, 0: none) selects the hop index
// (k_nl_hop: data line ends predicted from S and checked) over the full
// '\n' scan; its result must be confirmed by the encoder (VcfcEncodeArgs::nl_check).
// hop_walkers: walkers of the hop index (0: HOP_WALKERS; the tests use a few,
// so each walks as many lines as at config size).  hop_learn: the walkers
// learn the genotype-region lengths of lines that are not 3-byte tokens
// (TRY / LEARN, k_nl_hop<true>).  len_hint (!hop_learn; 0: none): a data
// line's length with its '\n' (the file's first): every walker but the
// first guesses its first lines from it (GUESS) instead of reading the
// first line's prefix.
// Learned candidates handed to every TRY / LEARN walker at its start (the
// host's: data lines of the file's first window whose genotype region is not
// 4 S - 1 bytes): region length g[k] (0: none) and, for each of the 16 lanes
// of a walker, the TAB mask of its 16 bytes of the 256 ending at the '\n'.
struct VcfcHopCands {
    uint32_t g[3];
    uint16_t sig[3][16];
};
hipError_t vcfc_line_index(const uint8_t *buf, uint64_t n, uint8_t *ws, const VcfcLineIndexLayout &L,
                           const VcfcLineIndex &x, hipStream_t s, uint32_t S_hint = 0, uint64_t hop_walkers = 0,
                           bool hop_learn = true, uint32_t len_hint = 0, const VcfcHopCands *cands = nullptr);
// phase 2 (n_lines = counts[0]): '\n' positions, data / pass line arrays; counts[1], counts[2]
hipError_t vcfc_line_index_place(const uint8_t *buf, uint64_t n, uint64_t n_lines, const uint8_t *ws1, uint8_t *ws2,
                                 const VcfcLineIndexLayout &L, const VcfcLineIndex &x, hipStream_t s);
// counts[0..3] and the first pk '#' line entries into out (32 + 24 pk bytes)
hipError_t vcfc_index_summary(const VcfcLineIndex &x, uint64_t pk, uint8_t *out, hipStream_t s);

// ---------------------------------------------------------------------------
// Binned external index (vcfc_index.hip; reference create_binned_index4,
// src/main.cpp:1284-1637, and query_binned_index_binarysearch, :2974-3349).
struct VcfcIndexLayout {
    uint64_t ref_idx, pos, end, pmax, flag, eno, bmax, partials, total;
};
VcfcIndexLayout vcfc_index_workspace_layout(uint64_t n);
// one lane per record [rec_start[i], rec_start[i + 1]): ref_idx (1..25 for
// "1".."22", "X", "Y", "M", else 0), POS and the end position
// (compute_end_position, :763-852); err = min over records of (i << 8 |
// code), code 2 = the reference throws (POS, an INFO pair, END or SVLEN does
// not parse), 3 = the first eight TABs do not all lie inside the record
hipError_t vcfc_index_span(const uint8_t *in, const uint64_t *rec_start, uint64_t n, uint8_t *ref_idx, uint64_t *pos,
                           uint64_t *end, uint64_t *err, hipStream_t s);
// span + prefix maximum + open flags + entry numbers + the packed 13-byte
// entries {u8 ref_idx, u32 position, u64 base_offset + rec_start[k]};
// *count = entries, *info = the largest end (the entries hold the
// reference's only while it is below 2^32); err as vcfc_index_span, and
// code 0xFF: an entry past entries_cap.  No host synchronisation.
hipError_t vcfc_index_build(const uint8_t *in, const uint64_t *rec_start, uint64_t n, uint64_t base_offset,
                            uint64_t entries_per_bin, uint8_t *entries, uint64_t entries_cap, uint64_t *count,
                            uint64_t *info, uint8_t *ws, const VcfcIndexLayout &L, uint64_t *err, hipStream_t s);
// compare_to_range (:110-137) per record: flag[i] = 1 where the record lies
// in the query; *first_after = the first record after it (~0: none)
hipError_t vcfc_index_compare(const uint8_t *ref_idx, const uint64_t *pos, const uint64_t *end, uint64_t n,
                              uint32_t qidx, uint64_t qstart, uint64_t qend, uint8_t *flag, uint64_t *first_after,
                              hipStream_t s);

// ---------------------------------------------------------------------------
// Sparse external index (vcfc_sparse_index.hip; reference
// create_sparse_external_index, src/main.cpp:854-999, and
// query_sparse_external_index, :1002-1281).
struct VcfcSparseIndexLayout {
    uint64_t ref_idx, pos, off, keep, eno, partials, total;
};
VcfcSparseIndexLayout vcfc_sparse_index_workspace_layout(uint64_t n);
// one lane per record: ref_idx and POS.  walk == 0: create's rules (five TABs
// inside the record; eight and compute_end_position's throws when ALT holds
// '<'); walk != 0: the query walk's (CHROM and POS only).  err = min over
// records of (i << 8 | code), code 2 = the reference throws, 3 = the TABs
// this action reads do not all lie inside the record
hipError_t vcfc_sparse_index_span(const uint8_t *in, const uint64_t *rec_start, uint64_t n, int walk, uint8_t *ref_idx,
                                  uint64_t *pos, uint64_t *err, hipStream_t s);
// span + slot offsets (300000000 + pos) * 256 + duplicate-slot resolution +
// the kept entries {u8 ref_idx, u32 pos, u64 base_offset + rec_start[i]} and
// their offsets, densely (entries: 13 n bytes, file_off: n words); *count =
// kept entries; status[1] = 1: some offset decreases (the kept set is not the
// reference's; write every record in order), status[2] = the first record
// whose offset is negative as off_t (~0: none).  No host synchronisation.
hipError_t vcfc_sparse_index_build(const uint8_t *in, const uint64_t *rec_start, uint64_t n, uint64_t base_offset,
                                   uint8_t *entries, uint64_t *file_off, uint64_t *count, uint64_t *status,
                                   uint8_t *ws, const VcfcSparseIndexLayout &L, uint64_t *err, hipStream_t s);
// gap-analysis (reference src/main.cpp:3931-3980), one lane per record: the
// location of the line's POS text (offset into `in`, length) and the
// reference's compressed count (line_byte_count, src/compress.cpp:764-968).
// err is NOT reset: atomicMin of (i << 8 | 3) for a record the walk refuses,
// so it shares the word of the decode plan that sizes the same records.
hipError_t vcfc_gap_fields(const uint8_t *in, const uint64_t *rec_start, uint64_t n, uint64_t S, uint64_t *pos_off,
                           uint32_t *pos_len, uint64_t *ccount, uint64_t *err, hipStream_t s);
