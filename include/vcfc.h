/*
 * vcfc.h -- C ABI of the MI355X-native `.vcfc` genotype-line codec
 * (libvcfc.so).  Plain pointers and sizes only; no C++ or torch types.
 *
 * Drop-in boundary.  The reference has no FFI: its only boundary for this
 * path is the C++ function
 *     int compress_data_line(const std::string& line,
 *                            const VcfCompressionSchema& schema,
 *                            std::vector<byte_t>& byte_vec, bool add_newline);
 * (reference src/compress.hpp:20-23, defined src/compress.cpp:5-203) whose
 * single caller is compress() (src/compress.cpp:205-257, call at :244).
 * vcfc_compress_data_line() is its one-line replacement; the batch entry
 * points below replace the compress() loop around it.  INTEGRATION.md shows
 * the shim a maintainer adds on the reference side.
 *
 * Output is byte-identical to the reference for every input line: records
 * [LEN][REQ][cols][GT][\n] concatenated in row order (format: reference
 * src/utils.hpp:44-56,140-247, src/compress.cpp:32-199).
 */
#ifndef VCFC_H
#define VCFC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------- */
#define VCFC_OK 0
/* VcfValidationError("VCF data line did not contain at least 8 terms"),
 * reference src/compress.cpp:9-11 */
#define VCFC_E_LT8COLS 1
/* exactly 8 terms: the reference's size_t underflow -> std::length_error ->
 * abort (src/compress.cpp:89,107); reported instead of aborting */
#define VCFC_E_8COLS 2
/* VcfValidationError("VCF Header did not have enough columns"),
 * src/compress.cpp:231-234 */
#define VCFC_E_HEADER 3
#define VCFC_E_NOSPACE 4   /* caller buffer too small */
#define VCFC_E_ARG 5       /* bad argument */
#define VCFC_E_HIP 6       /* HIP runtime error / no GPU */
#define VCFC_E_IO 7        /* file open/read/write failed */
#define VCFC_E_FORMAT 8    /* malformed .vcfc input (decoder) */
/* a data line longer than VCFC_MAX_LINE bytes: its record could pass the
 * 30-bit LEN header (LineLengthHeader's 2^30 - 1, reference
 * src/utils.hpp:140-160), which the reference would silently truncate */
#define VCFC_E_TOOLONG 10
#define VCFC_MAX_LINE ((1u << 29) - 64u)

const char *vcfc_version(void);
const char *vcfc_strerror(int status);

/* ---- context ----------------------------------------------------------------
 * One context per GPU (device ordinal); not shared across host threads.
 * Fails with VCFC_E_HIP when no GPU is visible: there is no CPU fallback. */
typedef struct vcfc_ctx vcfc_ctx;
int vcfc_ctx_create(int device, vcfc_ctx **out);
void vcfc_ctx_destroy(vcfc_ctx *ctx);
/* Input chunk of the pipelined file compress (vcfc_compress_file/_buffer):
 * chunk_bytes in [4096, 3 GiB], or 0 for the default (128 MiB).  A line longer
 * than the chunk grows that chunk (doubling) until it fits; no input is read
 * twice.  The reference reads line by line (getline, src/compress.cpp:218);
 * the output does not depend on the chunk size. */
int vcfc_ctx_set_ingest_chunk(vcfc_ctx *ctx, uint64_t chunk_bytes);
/* Line index of vcfc_compress_device: VCFC_LINE_INDEX_HOP (default) guesses
 * each data line's end from the header's sample count and checks it (a wrong
 * guess re-indexes the chunk from every byte, so the output never depends on
 * it); VCFC_LINE_INDEX_SCAN reads every byte.  The reference finds lines with
 * getline (src/compress.cpp:218). */
#define VCFC_LINE_INDEX_HOP 0
#define VCFC_LINE_INDEX_SCAN 1
int vcfc_ctx_set_line_index(vcfc_ctx *ctx, int mode);
/* Stage timings / decisions of the host drivers to stderr (diagnostics; off
 * by default): OR of the flags below. */
#define VCFC_TRACE_INGEST 1u        /* vcfc_compress_file/_buffer/_range: stage totals */
#define VCFC_TRACE_DEVICE 2u        /* vcfc_compress_device: chunks, sample count, re-indexes */
#define VCFC_TRACE_SPARSE_QUERY 4u  /* vcfc_sparse_query*: stage totals */
#define VCFC_TRACE_INDEX 8u         /* vcfc_query_binned_index*: windows / bytes read by the indexed query */
int vcfc_ctx_set_trace(vcfc_ctx *ctx, unsigned flags);
/* Deferred records (1 = on, the default since round 5; 0 = off) for the
 * context's file and device compress calls (vcfc_encode_rows_device and the
 * one-line / host-batch calls always use them): a row of odd-length tokens
 * whose first genotype chunk is all escapes (GT:DP:GQ and the like, records
 * ~1.1x their lines) and that spans more than one 2 KiB chunk is only sized
 * by the first pass and encoded straight into the output once the record
 * offsets are known, instead of staged and copied.  The choice is made per
 * row by the kernel from the row's bytes; once two rows agree on their token
 * count, a deferred row's size is predicted from its first chunk and checked
 * when it is written (a wrong guess lays the batch out again: three gated
 * launches that return at once otherwise).  Output identical either way
 * (DESIGN.md section 3). */
int vcfc_ctx_set_deferred_records(vcfc_ctx *ctx, int on);

/* ---- one line: replaces compress_data_line (src/compress.hpp:20-23) --------
 * Appends the record for `line` (no trailing '\n'; `len` bytes) to `out`
 * (capacity `out_cap`), writes its size to *out_len.  add_newline as in the
 * reference (compress() always passes true).  Returns VCFC_OK or an error;
 * nothing is written on error. */
int vcfc_compress_data_line(vcfc_ctx *ctx, const char *line, uint64_t len, int add_newline,
                            uint8_t *out, uint64_t out_cap, uint64_t *out_len);

/* ---- batches of lines ------------------------------------------------------
 * Upper bound of the encoded size of rows whose line bytes sum to
 * total_line_bytes (records only). */
uint64_t vcfc_encode_bound(uint64_t n_rows, uint64_t total_line_bytes);

/* Device workspace bytes needed by vcfc_encode_rows_device. */
uint64_t vcfc_encode_workspace_size(uint64_t n_rows, uint64_t total_line_bytes);

/* Device-resident batch encode, asynchronous on `stream` (a hipStream_t; 0 =
 * the default stream).  All pointers are device pointers.
 *   d_buf            data-line bytes
 *   d_line_off/len   line i = d_buf[d_line_off[i] .. + d_line_len[i]) (no '\n')
 *   d_out            records in row order; d_rec_off[0..n] exclusive offsets
 *                    (d_rec_off[n] = total bytes)
 *   d_ws             workspace of vcfc_encode_workspace_size(n, total) bytes
 *                    where total >= sum of d_line_len
 *   d_err            one uint64: ~0 = success, else (row << 8 | status) of the
 *                    first failing row (rows before it are valid output)
 * Output bytes: [0, d_rec_off[n]) hold the records; with deferred records a
 * call may also write stale bytes into [d_rec_off[n], out_cap) (records
 * placed on predicted offsets before a misprediction is found), never past
 * out_cap -- several batches that share one buffer go in row order.
 * Returns VCFC_OK if the work was enqueued.  Capturable in a hipGraph: the
 * per-call state is reset by a kernel, not by hipMemsetAsync -- on this ROCm
 * a captured 24-byte memset node writes garbage into its first 16 bytes from
 * the second replay on (4- and 8-byte nodes replay correctly;
 * tools/dbg/memset_graph_probe.py, profiles/r04/memset_graph_probe.txt).
 * The n == 0 call enqueues two 8-byte memsets (safe).  The host-driven entry
 * points below (vcfc_compress_*, the decoders) synchronise and are not meant
 * for capture. */
int vcfc_encode_rows_device(const uint8_t *d_buf, const uint64_t *d_line_off,
                            const uint32_t *d_line_len, uint64_t n, uint64_t total_line_bytes,
                            uint8_t *d_out, uint64_t out_cap, uint64_t *d_rec_off,
                            void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream);

/* Rows the last vcfc_encode_rows_device call on workspace d_ws (sized for
 * n, total_line_bytes) deferred and wrote straight into the output (see
 * vcfc_ctx_set_deferred_records; a row whose predicted size led there but
 * whose later bytes sent it to the general path, or that held a '\n' or
 * failed, is not counted); waits for `stream`. */
int vcfc_encode_deferred_rows(const void *d_ws, uint64_t n_rows, uint64_t total_line_bytes, void *stream,
                              uint64_t *rows);

/* Per-stage timing of vcfc_encode_rows_device (HIP events on the same
 * stream).  vcfc_timer_read synchronises and returns the per-stage totals in
 * ms summed over the timed calls since the last read:
 *   ms[0] slot-offset scan, ms[1] k_encode (the fast and variable-token
 *   kernels, plus k_encode_defer's deferred records after the compaction),
 *   ms[2] record-offset scan, ms[3] k_compact;  *calls = number of timed
 *   calls. */
typedef struct vcfc_timer vcfc_timer;
int vcfc_timer_create(vcfc_timer **t);
void vcfc_timer_destroy(vcfc_timer *t);
int vcfc_encode_rows_device_timed(const uint8_t *d_buf, const uint64_t *d_line_off,
                                  const uint32_t *d_line_len, uint64_t n, uint64_t total_line_bytes,
                                  uint8_t *d_out, uint64_t out_cap, uint64_t *d_rec_off,
                                  void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream,
                                  vcfc_timer *t);
int vcfc_timer_read(vcfc_timer *t, double ms[4], uint64_t *calls);

/* Host batch encode (synchronous: H2D, encode on the context's GPU, D2H).
 * rec_off has n + 1 entries.  On a failing row, returns its status and
 * *err_row = its index; records of the rows before it are in `out`. */
int vcfc_encode_rows(vcfc_ctx *ctx, const uint8_t *buf, uint64_t buf_bytes,
                     const uint64_t *line_off, const uint32_t *line_len, uint64_t n,
                     uint8_t *out, uint64_t out_cap, uint64_t *rec_off, int64_t *err_row);

/* ---- whole files: compress() / decompress2_fd() ---------------------------
 * compress: header ("##" and "#") lines pass through with '\n', empty lines
 * are skipped, data lines are encoded on the GPU (reference
 * src/compress.cpp:205-257).  On error returns the status and *err_line =
 * 1-based input line number. */
int vcfc_compress_file(vcfc_ctx *ctx, const char *in_path, const char *out_path, int64_t *err_line);
/* In-memory variant of vcfc_compress_file (out_cap >= vcfc_compress_bound). */
uint64_t vcfc_compress_bound(uint64_t in_bytes);
int vcfc_compress_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t n, uint8_t *out, uint64_t out_cap,
                         uint64_t *out_len, int64_t *err_line);

/* compress() over VCF file bytes already resident in device memory (a
 * pipeline stage that produced or received the file on the GPU): d_in[0, n)
 * holds the file's bytes as read, with n > 0 and d_in[n - 1] == '\n' (append
 * one to an unterminated last line: getline returns it, reference
 * src/compress.cpp:218); else VCFC_E_ARG.  The line index and the encoder run
 * on the context's GPU; the bytes compress() writes -- '#' lines verbatim in
 * place, records of the data lines -- land at d_out[0, *out_len) (out_cap >=
 * vcfc_compress_bound(n)).  Runs on the context's stream: complete the
 * writes of d_in first.  Synchronous (the host reads the index counts and
 * the '#' lines).  Statuses and *err_line as vcfc_compress_buffer; on a
 * failing line d_out holds the output of the lines before it. */
int vcfc_compress_device(vcfc_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t out_cap,
                         uint64_t *out_len, int64_t *err_line);

/* One rank's share of a multi-GPU compress (SURVEY §8 e): compresses the
 * byte range [off, off + len) of in_path (whole lines: off at a line start,
 * off + len after a '\n' or at EOF) through the same pipeline and writes the
 * output to out_fd at out_off onwards (pwrite; nothing else in the file is
 * touched).  *out_bytes = bytes written (on a failing line: the output of the
 * lines before it), *err_line = 1-based line within the range, *lines =
 * lines in the range (for global line numbers).  The concatenation of the
 * ranks' outputs in range order equals vcfc_compress_file's output (compress()
 * keeps no state across lines, reference src/compress.cpp:205-257). */
int vcfc_compress_range(vcfc_ctx *ctx, const char *in_path, uint64_t off, uint64_t len, int out_fd,
                        uint64_t out_off, uint64_t *out_bytes, int64_t *err_line, uint64_t *lines);

/* vcfc_compress_range with the output held for a later placement: the
 * rank's offset in the output file is the exclusive prefix of the ranks' byte
 * counts, known only after their all-gather.  The first mem_bound bytes stay
 * in host memory, the rest go to an unlinked temporary file in spill_dir
 * (NULL: /tmp).  vcfc_held_place writes all held bytes at out_off of out_fd
 * (memory blocks by pwrite, the spilled part by copy_file_range), so output
 * that fits in memory is written once, to its final place.  *held is set even
 * on a failing line (it holds the output of the lines before it); free it
 * with vcfc_held_free. */
typedef struct vcfc_held vcfc_held;
int vcfc_compress_range_held(vcfc_ctx *ctx, const char *in_path, uint64_t off, uint64_t len, uint64_t mem_bound,
                             const char *spill_dir, vcfc_held **held, uint64_t *out_bytes, int64_t *err_line,
                             uint64_t *lines);
int vcfc_held_place(const vcfc_held *held, int out_fd, uint64_t out_off);
/* bytes held in host memory / in the spill file */
void vcfc_held_sizes(const vcfc_held *held, uint64_t *mem_bytes, uint64_t *spill_bytes);
void vcfc_held_free(vcfc_held *held);

/* ---- decoder: decompress2_fd (reference src/compress.cpp:1214-1257,
 * decompress2_data_line :741-986) ----------------------------------------
 * .vcfc bytes -> VCF text, byte-identical to the reference's `main
 * decompress`.  The sample count comes from the header line (as in the
 * reference).  On VCFC_E_FORMAT (where the reference throws) the output holds
 * the header and every line the reference writes before throwing.
 * vcfc_decompress_buffer: VCFC_E_NOSPACE if out_cap is short; *out_len is
 * then the size needed. */
int vcfc_decompress_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t out_cap,
                           uint64_t *out_len);
int vcfc_decompress_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_vcf);

/* Device-resident batch: records d_in[d_rec_start[i], d_rec_start[i+1]) for
 * i < n (e.g. an encoder batch's rec_off), `samples` from the header line.
 * Enqueued on `stream` with no host synchronisation.  Lines land at
 * d_out + d_line_off[i] (n + 1 offsets, d_line_off[n] = total).  d_err:
 * ~0, or min over records of (i << 8 | 2) where a record's byte-serial parse
 * ends off its LEN (the file decoder then continues byte-serially) or
 * (i << 8 | 3) where the reference throws; such records get no line, and
 * lines past the first one are not meaningful.  (i << 8 | 0xFF): out_cap
 * too small.  exact = 0 plans from the headers and REQ bytes only and
 * assumes every sample section is "simple" (3-byte tokens, exactly
 * `samples` of them); the writer checks that and reports (i << 8 | 4) where
 * it was wrong: call again with exact = 1. */
uint64_t vcfc_decode_workspace_size(uint64_t n_records);
int vcfc_decode_records_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start, uint64_t n,
                               uint64_t samples, uint8_t *d_out, uint64_t out_cap, uint64_t *d_line_off,
                               void *d_ws, uint64_t ws_bytes, uint64_t *d_err, int exact, void *stream);
/* As vcfc_decode_records_device, for the records with d_select[i] != 0 only
 * (the others get no line: d_line_off[i + 1] == d_line_off[i]); d_select =
 * the range query's match flags (vcfc_query_match_device). */
int vcfc_decode_selected_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start,
                                const uint8_t *d_select, uint64_t n, uint64_t samples, uint8_t *d_out,
                                uint64_t out_cap, uint64_t *d_line_off, void *d_ws, uint64_t ws_bytes,
                                uint64_t *d_err, int exact, void *stream);

/* ---- range query: query_compressed_file (reference src/main.cpp:3777-3929)
 * Lines (no header) of the records whose CHROM equals `ref` (ref_len == 0:
 * any name) and, when has_range, whose POS lies in [start, end]
 * (VcfCoordinateQuery::matches, src/main.cpp:75-86), byte-identical to the
 * reference's stdout.  On VCFC_E_FORMAT (where the reference throws) the
 * output holds every line the reference writes before throwing.
 * vcfc_parse_query restates parse_coordinate_string (src/main.cpp:3993-4026):
 * "<ref>" or "<ref>:<start>-<end>"; returns 0, or 1 (no '-' after the ':'),
 * 2 (start does not parse), 3 (end does not parse) where the reference
 * prints its message and exits 1; *ref_len = bytes of q holding the name.
 * vcfc_query_buffer: VCFC_E_NOSPACE if out_cap is short (*out_len = size
 * needed); vcfc_query_file writes to out_fd as lines are decoded. */
int vcfc_parse_query(const char *q, uint64_t q_len, uint64_t *ref_len, int *has_range, uint64_t *start,
                     uint64_t *end);
int vcfc_query_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const char *ref, uint64_t ref_len,
                      int has_range, uint64_t start, uint64_t end, uint8_t *out, uint64_t out_cap,
                      uint64_t *out_len);
int vcfc_query_file(vcfc_ctx *ctx, const char *in_vcfc, const char *ref, uint64_t ref_len, int has_range,
                    uint64_t start, uint64_t end, int out_fd);
/* Device-resident match step: d_flag[i] = 1 where record
 * d_in[d_rec_start[i], d_rec_start[i+1]) matches; *d_err = ~0 or min over
 * records of (i << 8 | 2) where its POS does not parse (the reference
 * throws) or (i << 8 | 3) where CHROM/POS runs past the record (the
 * reference's walk leaves the LEN hops there).  d_ref is device memory.
 * Enqueued on `stream`; decode the flagged records with
 * vcfc_decode_selected_device. */
int vcfc_query_match_device(const uint8_t *d_in, const uint64_t *d_rec_start, uint64_t n, const uint8_t *d_ref,
                            uint64_t ref_len, int has_range, uint64_t start, uint64_t end, uint8_t *d_flag,
                            uint64_t *d_err, void *stream);

/* ---- binned external index: create_binned_index4 (reference
 * src/main.cpp:1284-1637, compute_end_position :763-852) and
 * query_binned_index_binarysearch (:2974-3349; CLI :4097-4143) --------------
 * The index of <file.vcfc> is <file.vcfc>.vcfci: packed 13-byte entries
 * {u8 ref_idx, u32 position (LE), u64 byte_offset (LE)} (struct index_entry,
 * :600-626).  ref_idx is 1..25 for CHROM "1".."22", "X", "Y", "M", else 0
 * (reference_name_map, src/utils.hpp:97-100); a record's end position is POS
 * + max(|REF|, longest ALT piece) - 1, or for an ALT holding '<' INFO's END,
 * else POS + max |SVLEN| - 1, else POS.  Record 0 opens an entry; record i
 * with i % entries_per_bin == 0 opens one iff its end passes the last
 * entry's position; every other record only raises that position
 * (:1436-1482).  byte_offset is the record's offset in the file (the
 * reference's ftell, header bytes included).
 *
 * One deviation: a record whose first eight TABs do not all lie inside it
 * (code 3) is refused with VCFC_E_FORMAT, where the reference reads on into
 * the next record; no file written by compress has such a record. */
#define VCFC_INDEX_ENTRY_BYTES 13
uint64_t vcfc_index_workspace_size(uint64_t n_records);
/* device-resident, async on stream: records d_in[d_rec_start[i], d_rec_start[i+1]),
 * byte_offset of record i = base_offset + d_rec_start[i]; *d_count = entries;
 * d_err as vcfc_query_match_device (codes 2, 3; 0xFF: entries_cap too small);
 * d_info[0] = max end (caller replays on the host when > 0xFFFFFFFF: the
 * reference then compares a 64-bit end with the entry's truncated u32
 * position, :1442-1466, and the entries written here are not its) */
int vcfc_binned_index_device(const uint8_t *d_in, const uint64_t *d_rec_start, uint64_t n, uint64_t base_offset,
                             uint64_t entries_per_bin, uint8_t *d_entries, uint64_t entries_cap, uint64_t *d_count,
                             uint64_t *d_info, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream);
/* per record: ref_idx, POS and the end position (compute_end_position,
 * :763-852); d_err as above (codes 2, 3) */
int vcfc_record_span_device(const uint8_t *d_in, const uint64_t *d_rec_start, uint64_t n, uint8_t *d_ref_idx,
                            uint64_t *d_pos, uint64_t *d_end, uint64_t *d_err, void *stream);
/* create_binned_index4 (:1284-1637) over .vcfc bytes / a file.
 * entries_per_bin == 0: VCFC_E_ARG (the reference dies of SIGFPE).  Where
 * the reference throws: VCFC_E_FORMAT, *err_record = the record, no index
 * bytes (the reference writes its entries only at the end, :1621-1628; the
 * file variant leaves <out_index> empty).  VCFC_E_NOSPACE: *out_len = bytes
 * needed. */
int vcfc_create_binned_index_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint64_t entries_per_bin,
                                    uint8_t *out, uint64_t out_cap, uint64_t *out_len, int64_t *err_record);
int vcfc_create_binned_index_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_index,
                                  uint64_t entries_per_bin);
/* query_binned_index_binarysearch (:2974-3349): the binary search of
 * :3047-3167 picks an entry, the walk of :3206-3329 starts at its
 * byte_offset and outputs the lines of the records that compare_to_range
 * (:110-137) places in (ref, start, end), up to the first record after it.
 * A bare name (has_range == 0) queries start = end = 0 as the reference
 * does.  An index whose size is not a multiple of 13: VCFC_E_FORMAT (the
 * reference throws, :3018-3022); no entries: no output; one entry (the
 * reference reads an uninitialised struct): entry 0.  Only the header and
 * the bytes from that byte_offset on are read.  The _buffer variant returns
 * VCFC_E_NOSPACE with *out_len = the size needed. */
int vcfc_query_binned_index_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const uint8_t *index,
                                   uint64_t index_bytes, const char *ref, uint64_t ref_len, int has_range,
                                   uint64_t start, uint64_t end, uint8_t *out, uint64_t out_cap, uint64_t *out_len);
int vcfc_query_binned_index_file(vcfc_ctx *ctx, const char *in_vcfc, const char *in_index, const char *ref,
                                 uint64_t ref_len, int has_range, uint64_t start, uint64_t end, int out_fd);

/* ---- sparse external index: create_sparse_external_index (reference
 * src/main.cpp:854-999; CLI :4144-4157) and query_sparse_external_index
 * (:1002-1281; CLI :4158-4177) ----------------------------------------------
 * The index of <file.vcfc> is <file.vcfc>.vcfci-sparse, a sparse file: the
 * entry of a record {u8 ref_idx, u32 (uint32)POS (LE), u64 byte_offset (LE)}
 * (the binned index's 13 packed bytes) lies at file offset (300000000 + POS)
 * * 256 in 64-bit wrap-around arithmetic (compute_sparse_offset,
 * src/sparse.cpp:18-51, with multiplication_factor 1 and block size 256;
 * CHROM is not part of it, VCFC_SPARSE_MULTIPLE_REF_PER_FILE being false).
 * The reference writes one entry per record in file order, so of the records
 * that share a slot the last one stays.  CHROM .. ALT are the bytes up to the
 * first five TABs; QUAL, FILTER and INFO are read only when ALT holds '<',
 * and compute_end_position (:763-852) then runs for its throws alone.
 *
 * One deviation: a record whose five (eight for a structural ALT) TABs do
 * not all lie inside it (code 3) is refused with VCFC_E_FORMAT, where the
 * reference reads on into the next record; no file written by compress has
 * such a record. */
uint64_t vcfc_sparse_index_workspace_size(uint64_t n_records);
/* compute_sparse_offset (src/sparse.cpp:18-51) for the index: the file
 * offset of the slot of `pos` */
uint64_t vcfc_sparse_index_offset(uint64_t pos);
/* device-resident, async on stream: records d_in[d_rec_start[i],
 * d_rec_start[i+1]), byte_offset of record i = base_offset + d_rec_start[i].
 * Of each run of records with equal slot offsets the last is kept; the kept
 * entries (13 bytes each) and their file offsets are written densely, in
 * record order, to d_entries (13 n bytes) and d_file_off (n words); *d_count
 * = kept entries.  d_status (3 words): [1] = 1 where some record's offset is
 * below its predecessor's -- the kept set is then not what the reference's
 * sequential writes leave, and the caller writes every record in order;
 * [2] = the first record whose offset is negative as off_t (the reference's
 * lseek fails there, :954-959), ~0 for none; [0] = 0.  d_err as
 * vcfc_binned_index_device (codes 2, 3). */
int vcfc_sparse_index_device(const uint8_t *d_in, const uint64_t *d_rec_start, uint64_t n, uint64_t base_offset,
                             uint8_t *d_entries, uint64_t *d_file_off, uint64_t *d_count, uint64_t *d_status,
                             void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream);
/* create_sparse_external_index (:854-999): <out_index> is opened O_CREAT |
 * O_TRUNC, mode 0600, before the input is parsed.  The run stops at the
 * first record the reference throws on (VCFC_E_FORMAT, *err_record = the
 * record; also for a record header it cannot read) or cannot seek to
 * (VCFC_OK, *seek_failed = 1: the reference prints "lseek: Invalid argument"
 * and exits 0); the entries of the records before it are in the file either
 * way.  A header without a data line: VCFC_E_FORMAT, *err_record = -1, the
 * index left empty.  err_record and seek_failed may be null. */
int vcfc_create_sparse_index_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_index, int64_t *err_record,
                                  int *seek_failed);
/* query_sparse_external_index (:1002-1281).  Lookup (:1040-1174): the
 * SEEK_DATA probe at offset 10000000 must find data (an index without an
 * entry: no output); the entry at the slot of `start` (a bare name,
 * has_range == 0, queries start = end = 0; CHROM is ignored); at or past
 * EOF: no output; an all-zero entry: no output when start == end, else the
 * first non-zero slot after it (SEEK_DATA, then steps of 256).  Walk
 * (:1191-1266): from the entry's byte_offset, records for which compare_to
 * (:88-108) places (CHROM, POS) before the query are skipped -- and, unlike
 * the reference, not decoded --, those inside it are output, the first one
 * after it ends the walk.  A POS that does not parse: VCFC_E_FORMAT after the
 * lines before it.  Only the header and the bytes from that byte_offset on
 * are read. */
int vcfc_query_sparse_index_file(vcfc_ctx *ctx, const char *in_vcfc, const char *in_index, const char *ref,
                                 uint64_t ref_len, int has_range, uint64_t start, uint64_t end, int out_fd);

/* ---- gap-analysis: gap_analysis (reference src/main.cpp:3931-3980) ---------
 * Line sizes without the lines: the decoder's exact plan (the sizing pass of
 * decompress2_data_line, src/compress.cpp:741-986) without its write pass.
 * d_line_off: n + 1 exclusive offsets of the decoded lines (LF included);
 * d_pos_off / d_pos_len: where each line's POS text (its second non-empty
 * TAB field) lies in d_in; d_ccount: the reference's compressed count
 * (line_byte_count, src/compress.cpp:764-968): the 8 header bytes, the
 * required columns and each sample-section byte read, the closing LF counted
 * only where it ends an uncompressed column.  The last three may all be
 * null.  d_err: ~0 or (i << 8 | code) of the first record the decoder
 * refuses (its codes 2, 3); entries from record i on are undefined.
 *
 * One deviation: a record whose POS text does not lie wholly in its required
 * columns -- fewer than two non-empty fields there, or the second one ended
 * by the columns' end with sample tokens after it -- is refused (code 3),
 * where the reference prints the field as it runs on into the sample tokens;
 * no file written by compress has such a record. */
uint64_t vcfc_decode_sizes_workspace_size(uint64_t n_records);
int vcfc_decode_sizes_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start, uint64_t n,
                             uint64_t sample_count, uint64_t *d_line_off, uint64_t *d_pos_off, uint32_t *d_pos_len,
                             uint64_t *d_ccount, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream);
/* gap_analysis (:3931-3980): writes <out_txt> (truncated first; the CLI
 * passes "start-positions.txt"), one line "<POS> <decoded line bytes>
 * <compressed count>\n" per record, POS verbatim.  Where the reference throws
 * (a header without a data line, a record the decoder refuses):
 * VCFC_E_FORMAT, the lines of the records before it written. */
int vcfc_gap_analysis_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_txt);

/* ---- sample subset: decompress-samples, query-samples (no
 * reference counterpart: the oracle is a cut of the reference's own decode) --
 * `cols`: K >= 1 distinct 0-based sample columns, each < S (the '#CHROM'
 * line's sample count), in output order.  The output header is every '##'
 * line, then the '#CHROM' line's first 9 fields and the chosen names.  A
 * record is regular when both length headers carry bits 11, REQ is
 * non-empty, inside the record, holds exactly 9 TABs and no NUL, the sample
 * section is a sequence of run bytes (a count of 0 yields nothing) and
 * escapes (tokens ended by TAB, the record's very last one by the closing
 * LF) whose token counts add up to exactly S with no item passing S, and
 * the LF after them is the record's last byte.  Its line is REQ, the chosen
 * tokens joined by TAB, LF.  The call stops with VCFC_E_FORMAT at the first
 * record that is not regular, or where the LEN hops stop with 8 or more
 * bytes left; the output holds the header and every line before it.
 * VCFC_E_FORMAT with nothing written for a header the decoder refuses;
 * VCFC_E_ARG with nothing written for K = 0, a column >= S, a column listed
 * twice.  The query variants write no header, match records exactly as
 * vcfc_query_buffer does and ask only matching records to be regular; a
 * match error (codes 2, 3 of vcfc_query_match_device) at record k stops
 * there with VCFC_E_FORMAT.  Buffer variants: VCFC_E_NOSPACE if out_cap is
 * short (*out_len = size needed); vcfc_query_samples_file writes to out_fd. */
int vcfc_decompress_samples_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const uint32_t *cols,
                                   uint64_t n_cols, uint8_t *out, uint64_t out_cap, uint64_t *out_len);
int vcfc_decompress_samples_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_vcf, const uint32_t *cols,
                                 uint64_t n_cols);
int vcfc_query_samples_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const char *ref, uint64_t ref_len,
                              int has_range, uint64_t start, uint64_t end, const uint32_t *cols, uint64_t n_cols,
                              uint8_t *out, uint64_t out_cap, uint64_t *out_len);
int vcfc_query_samples_file(vcfc_ctx *ctx, const char *in_vcfc, const char *ref, uint64_t ref_len, int has_range,
                            uint64_t start, uint64_t end, const uint32_t *cols, uint64_t n_cols, int out_fd);
/* Resolve a comma-separated list of sample names (names[0, names_len))
 * against the '#CHROM' line of a .vcfc (host bytes; the header is enough):
 * cols[0, *n_cols) in list order.  Where the header repeats a name its first
 * occurrence wins.  VCFC_E_ARG with *bad_off = the offset in `names` of a
 * name the header does not hold, or of the second listing of a name;
 * VCFC_E_NOSPACE if cols_cap is short (*n_cols = columns needed);
 * VCFC_E_FORMAT for a header the decoder refuses. */
int vcfc_sample_columns(const uint8_t *in, uint64_t in_bytes, const char *names, uint64_t names_len, uint32_t *cols,
                        uint64_t cols_cap, uint64_t *n_cols, uint64_t *bad_off);
/* Device-resident subset decode, exact in one call: the lines of records
 * d_in[d_rec_start[i], d_rec_start[i+1]) (d_select nullable: records with
 * d_select[i] == 0 get no line and are not checked) at d_out +
 * d_line_off[i]; d_line_off[n] = total.  `cols` is host memory: it is
 * checked (VCFC_E_ARG as above, also for samples >= 2^31), sorted and
 * uploaded into the workspace before the kernels are enqueued on `stream`
 * (the upload synchronises the stream once).  As in the decoder, records
 * are loaded in whole dwords: up to 3 bytes past the last record's end must
 * be readable.  *d_err = ~0, or min over
 * records of (i << 8 | 3) where a record is not regular (it and the records
 * after it have no meaningful line), (i << 8 | 0xFF): out_cap too small. */
uint64_t vcfc_subset_workspace_size(uint64_t n_records, uint64_t n_cols);
int vcfc_decode_samples_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start,
                               const uint8_t *d_select, uint64_t n, uint64_t samples, const uint32_t *cols,
                               uint64_t n_cols, uint8_t *d_out, uint64_t out_cap, uint64_t *d_line_off, void *d_ws,
                               uint64_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- genotype counts: genotype-counts (no reference action:
 * the oracle is a tally over the reference's own decode) ---------------------
 * Counts taken from the run-length code without decoding it.  S is the
 * '#CHROM' line's sample count; S == 0 or S >= 2^30 is VCFC_E_ARG and a
 * header the decoder refuses VCFC_E_FORMAT, both with nothing written.
 * Records are found by LEN hops.  Without a query every record is counted,
 * and the call stops with VCFC_E_FORMAT at the first record that is not
 * regular (as defined above for the sample subset), or where hopping stops
 * with 8 or more bytes left.  With a query, records are matched exactly as
 * vcfc_query_buffer matches them; only matching records are counted and need
 * to be regular; a match error at record k stops there with VCFC_E_FORMAT.
 *
 * Per counted record, one row of eight uint32:
 *   n00 n01 n10 n11 n_other AN AC1 AC_other
 * n00 .. n11: the tokens that are exactly 0|0, 0|1, 1|0, 1|1 (run bytes by
 * class, and any escaped token that spells one of the four); n_other: every
 * other token; the five add up to S.  AN / AC1 / AC_other come from each
 * token's GT subfield under one total rule: GT is the token up to its first
 * ':' (or the whole token); it is split at every '|' and '/' (an empty GT is
 * one empty piece); a piece of one or more ASCII digits is a called allele of
 * class v = min(2, 10 v + d) folded over its digits from 0 (0, 00 -> 0; 1, 01
 * -> 1; 2, 10, 010 -> 2); every other piece is missing and counted nowhere.
 * AN = called alleles, AC1 = those of class 1, AC_other = those of class 2.
 * With S < 2^30 and records below 2^31 bytes nothing overflows 32 bits.
 * Per sample j < S, five uint64 c00 c01 c10 c11 c_other: the counted records
 * whose token j falls in each class.
 *
 * Device entry: the records d_in[d_rec_start[i], d_rec_start[i+1]), i < n <
 * 2^32 (d_select nullable: records with d_select[i] == 0 get a zero row and
 * are neither counted nor checked), read once.  d_variant (nullable, 16-byte
 * aligned): 8 n uint32, row i for record i.  d_sample (nullable): 5 samples
 * uint64, sample-major, ADDED to: the caller zeroes it, so batches and files
 * accumulate.  Asynchronous on `stream`, no host synchronisation.  *d_err =
 * ~0, or the minimum over records of (i << 8 | 3) where a record is not
 * regular: rows from record i on and the whole sample table are then not
 * meaningful.  VCFC_E_ARG: both outputs null, samples == 0 or >= 2^30, n >=
 * 2^32, ws_bytes below vcfc_counts_workspace_size(n, samples).  As in the
 * decoder, up to 3 bytes past the last record's end
 * must be readable.  vcfc_counts_lds_samples(): the largest `samples` whose
 * histogram is summed in LDS (above it the general path takes global
 * atomics).  vcfc_counts_trip_records(samples, with_sample_table): the records
 * one pass of the scan's resident grid covers on the current device, with or
 * without d_sample (a longer call goes round the grid again; 0 where the
 * device cannot be asked): for tests and tuning, no argument depends on it. */
uint64_t vcfc_counts_workspace_size(uint64_t n_records, uint64_t samples);
uint64_t vcfc_counts_lds_samples(void);
uint64_t vcfc_counts_trip_records(uint64_t samples, int with_sample_table);
int vcfc_genotype_counts_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start,
                                const uint8_t *d_select, uint64_t n, uint64_t samples, uint32_t *d_variant,
                                uint64_t *d_sample, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream);
/* A whole .vcfc in host memory.  has_query == 0: every record (ref .. end are
 * ignored).  rec_index[0, *n_rows) = the counted records' file indices and
 * rows[8 r ..] their rows: VCFC_E_NOSPACE if rows_cap is short (*n_rows =
 * rows needed).  sample_table: 5 S uint64, VCFC_E_NOSPACE if sample_cap (in
 * samples) is below S (*n_samples = S).  On VCFC_E_FORMAT the rows before the
 * failing record are returned, *err_record is its file index (the record
 * count where hopping stopped short) and the sample table is not written. */
int vcfc_genotype_counts_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, int has_query, const char *ref,
                                uint64_t ref_len, int has_range, uint64_t start, uint64_t end, uint64_t *rec_index,
                                uint32_t *rows, uint64_t rows_cap, uint64_t *n_rows, uint64_t *sample_table,
                                uint64_t sample_cap, uint64_t *n_samples, uint64_t *err_record);
/* Both outputs are opened (created, truncated) before the input is parsed.
 * variants_tsv: "#CHROM\tPOS\tN_00\tN_01\tN_10\tN_11\tN_OTHER\tAN\tAC1\t
 * AC_OTHER\n", then per counted record REQ's first two TAB fields verbatim
 * and the eight numbers in decimal, TAB-separated.  samples_tsv:
 * "#SAMPLE\tN_00\tN_01\tN_10\tN_11\tN_OTHER\n", then per sample its name
 * verbatim from the '#CHROM' line and the five numbers.  On VCFC_E_FORMAT
 * past the header the variants file holds its header line and the lines
 * before the failing record, and the samples file stays empty. */
int vcfc_genotype_counts_file(vcfc_ctx *ctx, const char *in_vcfc, const char *variants_tsv, const char *samples_tsv,
                              int has_query, const char *ref, uint64_t ref_len, int has_range, uint64_t start,
                              uint64_t end);

/* ---- region-list queries: one match pass over a whole BED /
 * region file.  No reference counterpart.
 * A region is what vcfc_parse_query yields; a record matches a region as the
 * range query decides (an empty name matches any CHROM, no range matches any
 * POS, else start <= POS <= end with POS parsed as there), and it matches a
 * region set iff it matches one of its regions: the flags are the OR of
 * vcfc_query_match_device's flags over the regions, the error word is
 * vcfc_query_match_device's.  A region with start > end matches nothing; so
 * does an empty set, which is not an error.  Output is in file order, each
 * record at most once.
 * Region text: one region per line.  LF ends a line, a CR before the LF is
 * dropped, the last line may lack its LF.  Lines that are empty or start
 * with '#', "track" or "browser" are skipped.  A line holding a TAB is BED,
 * name TAB start TAB end [TAB ...], start and end 1..20 ASCII digits that fit
 * 64 bits: the region name:[start + 1, end] (0-based, half-open; end <= start
 * is an empty region).  Any other line goes whole to vcfc_parse_query.
 * vcfc_regions_build writes the table, a position-independent blob (sorted
 * distinct names; per name its intervals sorted by start, overlapping and
 * adjacent ones merged; empty regions dropped).  VCFC_E_NOSPACE if table_cap
 * is short (*table_bytes = the size needed); VCFC_E_ARG with *bad_line = the
 * 1-based number of the first line that does not parse, or with *bad_line =
 * 0 for a table of 4 GiB or more.  *n_regions = parsed regions, empty ones
 * included. */
int vcfc_regions_build(const char *text, uint64_t len, uint8_t *table, uint64_t table_cap, uint64_t *table_bytes,
                       uint64_t *n_regions, uint64_t *bad_line);
/* Device-resident match step.  vcfc_regions_upload validates the host table
 * (magic word, counts and offsets inside table_bytes, names and starts
 * sorted; anything else, or ws_bytes below vcfc_regions_workspace_size, is
 * VCFC_E_ARG) and copies it into d_ws; the copy has left `table` when it
 * returns.  vcfc_regions_match_device is vcfc_query_match_device with the
 * uploaded table in place of one region: same d_flag, same *d_err; it is
 * enqueued on `stream` without host synchronisation, resets *d_err in a
 * kernel (capturable) and trusts what vcfc_regions_upload put into d_ws.
 * n == 0 and an empty table are valid. */
uint64_t vcfc_regions_workspace_size(uint64_t table_bytes);
int vcfc_regions_upload(const uint8_t *table, uint64_t table_bytes, void *d_ws, uint64_t ws_bytes, void *stream);
int vcfc_regions_match_device(const uint8_t *d_in, const uint64_t *d_rec_start, uint64_t n, const void *d_ws,
                              uint64_t ws_bytes, uint8_t *d_flag, uint64_t *d_err, void *stream);
/* A whole .vcfc against a built table (VCFC_E_ARG for a table
 * vcfc_regions_upload would refuse).  vcfc_query_regions_*: the full lines
 * (no header) of the matching records through the exact decoder.  The call
 * stops with VCFC_E_FORMAT at the first record with a match error, and at the
 * first matching record for which the decoder reports any error word; the
 * lines of the matching records before it are written.  After all lines it
 * returns VCFC_E_FORMAT where the LEN hops stop with 8 or more bytes left.
 * It does not take the byte-serial continuation of the reference's walk:
 * this action has no reference counterpart, so on a malformed file there is
 * nothing to reproduce.  NOSPACE and file opening as vcfc_query_buffer /
 * _file. */
int vcfc_query_regions_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const uint8_t *table,
                              uint64_t table_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_len);
int vcfc_query_regions_file(vcfc_ctx *ctx, const char *in_vcfc, const uint8_t *table, uint64_t table_bytes, int out_fd);
/* vcfc_query_samples_* with a table in place of the region: only matching
 * records need to be regular; a match error at record k stops there with
 * VCFC_E_FORMAT; VCFC_E_NOSPACE, VCFC_E_ARG and file opening as there. */
int vcfc_query_samples_regions_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const uint8_t *table,
                                      uint64_t table_bytes, const uint32_t *cols, uint64_t n_cols, uint8_t *out,
                                      uint64_t out_cap, uint64_t *out_len);
int vcfc_query_samples_regions_file(vcfc_ctx *ctx, const char *in_vcfc, const uint8_t *table, uint64_t table_bytes,
                                    const uint32_t *cols, uint64_t n_cols, int out_fd);
/* vcfc_genotype_counts_* with has_query = 1 and a table in place of the
 * region: only matching records are counted and need to be regular; a match
 * error at record k stops there with VCFC_E_FORMAT; outputs as there. */
int vcfc_genotype_counts_regions_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const uint8_t *table,
                                        uint64_t table_bytes, uint64_t *rec_index, uint32_t *rows, uint64_t rows_cap,
                                        uint64_t *n_rows, uint64_t *sample_table, uint64_t sample_cap,
                                        uint64_t *n_samples, uint64_t *err_record);
int vcfc_genotype_counts_regions_file(vcfc_ctx *ctx, const char *in_vcfc, const char *variants_tsv,
                                      const char *samples_tsv, const uint8_t *table, uint64_t table_bytes);

/* ---- genotype matrix: export-bed (no reference action: the
 * oracle is a per-token rule over the reference's own decode) ----------------
 * The variants x samples matrix written out of the run-length code, one row
 * per record.  Header, LEN hops, regular records, queries and the stop rules
 * are those of genotype-counts above.  One total rule per decoded token, on
 * the GT rule of genotype-counts (GT up to the first ':', split at every '|'
 * and '/', a piece of digits is called with class min(2, value), every other
 * piece is missing):
 *   dosage (int8)   -1 if any piece is missing, else the number of pieces
 *                   whose class is not 0, capped at 127
 *   hap (int8 pair) hk = the class of piece k if it exists and is called,
 *                   else -1; pieces past the second are ignored
 *   bed (2 bits)    exactly two pieces, both called, both of class 0 or 1:
 *                   0b11 for 0 and 0, 0b10 for one of each, 0b00 for 1 and 1;
 *                   every other token 0b01 (missing).  PLINK 1 with A1 = ALT,
 *                   A2 = REF.
 * Row layouts, for S samples (vcfc_matrix_row_bytes; 0 for an unknown layout):
 *   VCFC_GM_DOSAGE  S bytes, byte j = sample j
 *   VCFC_GM_HAP     2 S bytes, bytes 2j and 2j + 1 = h0 and h1 of sample j
 *   VCFC_GM_BED     ceil(S / 4) bytes, sample j in bits 2 (j mod 4) and
 *                   2 (j mod 4) + 1 of byte j / 4; the unused high bits of the
 *                   last byte are 0
 *
 * Device entry: the records d_in[d_rec_start[i], d_rec_start[i+1]), i < n <
 * 2^32, read once; d_select nullable: records with d_select[i] == 0 get no
 * row and are not checked.  d_row_of: n + 1 words, written on the device:
 * d_row_of[i] = the selected records before i (i without d_select),
 * d_row_of[n] = the number of rows.  The row of record i lies at d_out +
 * d_row_of[i] * row_stride; its bytes [row_bytes, row_stride) and every other
 * byte outside the rows are left untouched, for any stride and alignment.
 * Asynchronous on `stream`, no host synchronisation; per-call state is reset
 * by a kernel, so the call can be captured in a graph.  *d_err = ~0, or the
 * minimum over records of (i << 8 | 3) for a selected record that is not
 * regular (rows from i on are then not meaningful) and of (i << 8 | 0xFF) for
 * a record whose row would end past out_cap: that record and later ones are
 * not written, and nothing is ever written at or past d_out + out_cap.
 * VCFC_E_ARG: an unknown layout, samples == 0 or >= 2^30, n >= 2^32,
 * row_stride < row_bytes, a null d_out or d_row_of, ws_bytes below
 * vcfc_matrix_workspace_size(n, samples, layout).  Up to 3 bytes past the
 * last record's end must be readable.  vcfc_matrix_lds_samples(layout): the
 * largest `samples` whose row is put together in LDS (above it a byte-serial
 * path writes straight to global memory: correct, untuned).
 * vcfc_matrix_trip_records(layout): the records one pass of that kernel's
 * resident grid covers on the current device (a longer call goes round the
 * grid again; 0 for an unknown layout or where the device cannot be asked). */
#define VCFC_GM_DOSAGE 0
#define VCFC_GM_HAP 1
#define VCFC_GM_BED 2
uint64_t vcfc_matrix_row_bytes(int layout, uint64_t samples);
uint64_t vcfc_matrix_lds_samples(int layout);
uint64_t vcfc_matrix_trip_records(int layout);
uint64_t vcfc_matrix_workspace_size(uint64_t n_records, uint64_t samples, int layout);
int vcfc_genotype_matrix_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start,
                                const uint8_t *d_select, uint64_t n, uint64_t samples, int layout, uint8_t *d_out,
                                uint64_t out_cap, uint64_t row_stride, uint64_t *d_row_of, void *d_ws, uint64_t ws_bytes,
                                uint64_t *d_err, void *stream);
/* A whole .vcfc in host memory.  has_query == 0: every record (ref .. end are
 * ignored).  rec_index[0, *n_rows) = the rows' records' file indices (room
 * for rows_cap of them), rows = the matrix with row_stride = row_bytes (room
 * for rows_bytes bytes), *n_samples = S.  VCFC_E_NOSPACE if either is short:
 * *n_rows and *n_samples then give the sizes needed.  On VCFC_E_FORMAT the
 * rows before the failing record are returned and *err_record is its file
 * index (the record count where hopping stopped short).  The _regions entry
 * takes a built table (vcfc_regions_build) in place of the region. */
int vcfc_genotype_matrix_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, int layout, int has_query,
                                const char *ref, uint64_t ref_len, int has_range, uint64_t start, uint64_t end,
                                uint64_t *rec_index, uint64_t rows_cap, uint8_t *rows, uint64_t rows_bytes,
                                uint64_t *n_rows, uint64_t *n_samples, uint64_t *err_record);
int vcfc_genotype_matrix_regions_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, int layout,
                                        const uint8_t *table, uint64_t table_bytes, uint64_t *rec_index, uint64_t rows_cap,
                                        uint8_t *rows, uint64_t rows_bytes, uint64_t *n_rows, uint64_t *n_samples,
                                        uint64_t *err_record);
/* PLINK 1 files <out_prefix>.bed / .bim / .fam.  All three are opened
 * (created, truncated) before the input is parsed.  .bed: the bytes 6C 1B 01,
 * then the VCFC_GM_BED rows.  .bim: per row "CHROM\tID\t0\tPOS\tALT\tREF\n",
 * REQ's TAB fields 0, 2, 1, 4, 3 verbatim.  .fam: per sample
 * "name\tname\t0\t0\t0\t-9\n", the names verbatim from the '#CHROM' line.  On
 * VCFC_E_FORMAT past the header .bed and .bim hold what precedes the failing
 * record and .fam stays empty; a header that is refused leaves all three
 * empty. */
int vcfc_export_bed_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_prefix, int has_query, const char *ref,
                         uint64_t ref_len, int has_range, uint64_t start, uint64_t end);
int vcfc_export_bed_regions_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_prefix, const uint8_t *table,
                                 uint64_t table_bytes);

/* ---- LD window: ld-window, ld-window-regions (no reference
 * action: the oracle is a plain restatement over the .bed rows) ----------------
 * Pairwise genotype tables of nearby rows of the genotype matrix.  The rows
 * are vcfc_genotype_matrix_*'s (every record, or the records a region or a
 * region table matches; dense, in file order; the same regular-record and
 * stop rules), and the window is in row space.  The genotype of a sample in a
 * row is its VCFC_GM_BED code: 11 -> 0, 10 -> 1, 00 -> 2, 01 -> missing;
 * columns >= samples do not exist.  For rows i < j, t[3 a + b] = the samples
 * with g_i = a and g_j = b, both called: nine uint32.  With window = W >= 1,
 * slot i * W + (k - 1) holds the table of rows (i, i + k), k = 1..W, and nine
 * zeros where row i + k does not exist; nothing outside slots [0, rows * W)
 * is written.  r2 of a table, with N = sum t, Sx = sum a t, Sy = sum b t,
 * Sxx = sum a^2 t, Syy = sum b^2 t, Sxy = sum a b t (exact in int64): cov =
 * N Sxy - Sx Sy, vx = N Sxx - Sx^2, vy = N Syy - Sy^2; undefined where vx == 0
 * or vy == 0, else ((double)cov * (double)cov) / ((double)vx * (double)vy).
 * The device delivers the integers only.
 *
 * vcfc_ld_tables_device: the pair step on .bed rows the caller holds (row r at
 * d_bed + r * row_stride, any row_stride >= row_bytes, any alignment; the
 * aligned 4-byte words that hold a row's bytes are read).  d_tables: 4-byte
 * aligned.  *d_err = ~0, or (r << 8 | 0xFF) where n_rows * window >
 * pairs_cap: r = pairs_cap / window is the first row that is not written
 * (a row's slots are written all or none), and nothing is written at or past
 * slot pairs_cap.  vcfc_ld_window_device: the composed call on device-resident
 * records, arguments as vcfc_genotype_matrix_device's: that call (layout
 * VCFC_GM_BED) writes the rows into the workspace, then bit planes, then
 * pairs, all enqueued on `stream` with no host synchronisation and per-call
 * state reset by a kernel (capturable).  d_row_of as there (n + 1 words).
 * *d_err is the matrix call's word: (i << 8 | 3) for a selected record that is
 * not regular -- tables that touch rows >= d_row_of[i] are then not
 * meaningful --, min'ed with (i << 8 | 0xFF) for the first record i whose
 * row's slots do not all fit pairs_cap.  VCFC_E_ARG: window == 0 or >= 2^16,
 * samples == 0 or >= 2^30, n (n_rows) >= 2^32, row_stride < row_bytes, a null
 * d_tables, d_row_of, d_ws or d_err, ws_bytes below
 * vcfc_ld_workspace_size(n, samples, window). */
uint64_t vcfc_ld_workspace_size(uint64_t n_records, uint64_t samples, uint64_t window);
int vcfc_ld_tables_device(const uint8_t *d_bed, uint64_t n_rows, uint64_t row_stride, uint64_t samples, uint64_t window,
                          uint32_t *d_tables, uint64_t pairs_cap, void *d_ws, uint64_t ws_bytes, uint64_t *d_err,
                          void *stream);
int vcfc_ld_window_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start, const uint8_t *d_select,
                          uint64_t n, uint64_t samples, uint64_t window, uint32_t *d_tables, uint64_t pairs_cap,
                          uint64_t *d_row_of, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream);
/* A whole .vcfc in host memory.  rec_index[0, *n_rows) = the rows' records'
 * file indices (room for rows_cap), tables = the band, *n_rows * window slots
 * of nine words (room for pairs_cap slots).  VCFC_E_NOSPACE if either is
 * short: *n_rows then gives the rows.  On VCFC_E_FORMAT the result is exactly
 * the band of the rows before the failing record, as if the file ended there,
 * and *err_record is its file index (the record count where hopping stopped
 * short).  The _regions entry takes a built table (vcfc_regions_build). */
int vcfc_ld_window_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint64_t window, int has_query,
                          const char *ref, uint64_t ref_len, int has_range, uint64_t start, uint64_t end,
                          uint64_t *rec_index, uint64_t rows_cap, uint32_t *tables, uint64_t pairs_cap, uint64_t *n_rows,
                          uint64_t *err_record);
int vcfc_ld_window_regions_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, uint64_t window,
                                  const uint8_t *table, uint64_t table_bytes, uint64_t *rec_index, uint64_t rows_cap,
                                  uint32_t *tables, uint64_t pairs_cap, uint64_t *n_rows, uint64_t *err_record);
/* out_tsv is opened (created, truncated) before the input is parsed.  The line
 * "#CHROM_A\tPOS_A\tID_A\tCHROM_B\tPOS_B\tID_B\tN\tR2\n", then one line per
 * written pair in slot order: REQ's TAB fields 0, 1, 2 of both records
 * verbatim, N in decimal, r2 as printf's %.6g or "nan" where it is undefined.
 * A pair whose CHROM fields differ bytewise is skipped.  min_r2 > 0: a pair is
 * written iff r2 is defined and r2 >= min_r2; min_r2 <= 0: every same-CHROM
 * pair is written.  On VCFC_E_FORMAT past the header the pairs among the rows
 * before the failing record are written; a header that is refused leaves the
 * file empty. */
int vcfc_ld_window_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_tsv, uint64_t window, double min_r2,
                        int has_query, const char *ref, uint64_t ref_len, int has_range, uint64_t start, uint64_t end);
int vcfc_ld_window_regions_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_tsv, uint64_t window, double min_r2,
                                const uint8_t *table, uint64_t table_bytes);

/* ---- kinship: kinship, kinship-regions (no reference action:
 * the oracle is a plain restatement over the .bed rows) ------------------------
 * Pairwise genotype tables of the samples over the rows of the genotype
 * matrix.  The rows are vcfc_genotype_matrix_*'s (every record, or the records
 * a region or a region table matches; the same regular-record and stop rules);
 * the genotype of sample s in a row is its VCFC_GM_BED code: 11 -> 0, 10 -> 1,
 * 00 -> 2, 01 -> missing; pad bits are never counted.  For samples i, j,
 * t[i][j][3 a + b] = the rows with g_i = a and g_j = b, both called: nine
 * uint32 at (i * samples + j) * 9, the full square (t[j][i] is the transpose,
 * t[i][i] is diagonal: the sample's own called genotype counts).  Statistics
 * of a table, exact in int64: N = sum t, IBS0 = t[2] + t[6], IBS2 = t[0] + t[4]
 * + t[8], IBS1 = N - IBS0 - IBS2, HH = t[4], HET_A = t[3] + t[4] + t[5], HET_B =
 * t[1] + t[4] + t[7], m = min(HET_A, HET_B); DST = (double)(2 IBS2 + IBS1) /
 * (double)(2 N), undefined for N == 0; KINSHIP (KING-robust, between families)
 * = (double)(2 HH - 4 IBS0 + 2 m - HET_A - HET_B) / (double)(4 m), undefined for
 * m == 0.  The device delivers the integers only.
 *
 * vcfc_kin_tables_device: the pair step on .bed rows the caller holds (row r at
 * d_bed + r * row_stride, any row_stride >= row_bytes, any alignment; the
 * aligned 4-byte words that hold a row's bytes are read).  d_tables: 4-byte
 * aligned, room for tables_cap >= samples^2 tables; d_ws: 16-byte aligned (the
 * bit planes in it are read 16 bytes at a time; hipMalloc gives 256), in both
 * device entries; accumulate != 0 adds to
 * what it holds (tables are additive over rows), else the square is stored.
 * *d_err = ~0.  vcfc_kin_records_device: the composed call on device-resident
 * records, arguments as vcfc_genotype_matrix_device's: that call (layout
 * VCFC_GM_BED) writes the rows into the workspace, then bit planes, then
 * pairs, all enqueued on `stream` with no host synchronisation and per-call
 * state reset by a kernel (capturable).  d_row_of as there (n + 1 words).
 * *d_err is the matrix call's word: with (i << 8 | 3), a selected record that
 * is not regular, the tables are exactly those of the rows [0, d_row_of[i])
 * before it.  VCFC_E_ARG, nothing written: samples == 0 or >= 2^30, n (n_rows)
 * >= 2^32, row_stride < row_bytes, tables_cap < samples^2, a null d_tables,
 * d_row_of, d_ws or d_err, ws_bytes below vcfc_kin_workspace_size(n, samples). */
uint64_t vcfc_kin_workspace_size(uint64_t n_records, uint64_t samples);
int vcfc_kin_tables_device(const uint8_t *d_bed, uint64_t n_rows, uint64_t row_stride, uint64_t samples, uint32_t *d_tables,
                           uint64_t tables_cap, int accumulate, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream);
int vcfc_kin_records_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start, const uint8_t *d_select,
                            uint64_t n, uint64_t samples, uint32_t *d_tables, uint64_t tables_cap, int accumulate,
                            uint64_t *d_row_of, void *d_ws, uint64_t ws_bytes, uint64_t *d_err, void *stream);
/* A whole .vcfc in host memory, in batches of records that add into one
 * square.  rec_index[0, *n_rows) = the rows' records' file indices (room for
 * rows_cap), tables = the *n_samples^2 tables (room for tables_cap tables).
 * VCFC_E_NOSPACE if either is short: *n_rows and *n_samples then give the
 * sizes.  On VCFC_E_FORMAT the result is exactly the square of the rows before
 * the failing record, as if the file ended there, and *err_record is its file
 * index (the record count where hopping stopped short).  The _regions entry
 * takes a built table (vcfc_regions_build). */
int vcfc_kinship_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, int has_query, const char *ref, uint64_t ref_len,
                        int has_range, uint64_t start, uint64_t end, uint64_t *rec_index, uint64_t rows_cap, uint32_t *tables,
                        uint64_t tables_cap, uint64_t *n_rows, uint64_t *n_samples, uint64_t *err_record);
int vcfc_kinship_regions_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const uint8_t *table,
                                uint64_t table_bytes, uint64_t *rec_index, uint64_t rows_cap, uint32_t *tables,
                                uint64_t tables_cap, uint64_t *n_rows, uint64_t *n_samples, uint64_t *err_record);
/* out_tsv is opened (created, truncated) before the input is parsed.  The line
 * "#ID_A\tID_B\tN\tIBS0\tIBS1\tIBS2\tHETHET\tHET_A\tHET_B\tDST\tKINSHIP\n",
 * then one line per written pair i < j, i ascending, then j: the two sample
 * names verbatim from the '#CHROM' line, the seven integers in decimal, DST and
 * KINSHIP as printf's %.6g or "nan" where undefined.  has_min != 0: a pair is
 * written iff its kinship is defined and >= min_kinship; else every pair.  On
 * VCFC_E_FORMAT past the header the pairs of the rows before the failing
 * record are written; a header that is refused leaves the file empty. */
int vcfc_kinship_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_tsv, int has_min, double min_kinship,
                      int has_query, const char *ref, uint64_t ref_len, int has_range, uint64_t start, uint64_t end);
int vcfc_kinship_regions_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_tsv, int has_min, double min_kinship,
                              const uint8_t *table, uint64_t table_bytes);

/* ---- extract: extract-samples, extract-regions (no reference
 * action: the oracle is the reference's own compress of the cut text) ----------
 * A sample / region subset of a .vcfc, written as a .vcfc; no record becomes
 * text.  `cols` as in the sample subset above (K >= 1 distinct columns < S, in
 * output order); cols == NULL with n_cols == 0 means all S columns in file
 * order.  The query is absent (has_query == 0), one region (matched exactly
 * as vcfc_query_samples_buffer matches) or a region table (vcfc_regions_build;
 * matched as vcfc_query_samples_regions_buffer matches).
 * The header is always written: every '##' line verbatim, then the '#CHROM'
 * line cut as the sample subset cuts it (verbatim with no column list).
 * Records are found by LEN hops; without a query every record is taken, with
 * one the matching records.  A taken record must be regular (the sample
 * subset's definition) and re-encodable: REQ's first byte is neither TAB nor
 * '#', REQ's last byte is TAB, REQ holds no two adjacent TABs, no chosen token
 * is empty, and the output record's LEN fits its 30 bits.  The output record
 * is exactly what the reference's compress writes for the line "REQ, chosen
 * tokens joined by TAB, LF": REQ verbatim; the chosen tokens re-coded greedily
 * in output order -- a token that spells 0|0 joins a run of up to 127, one
 * that spells 0|1, 1|0 or 1|1 a run of up to 31, full bytes first and the
 * remainder last, however the token was stored (an escape that spells a class
 * joins the run; source runs made adjacent by the cut merge) --, every other
 * token as 0xE1, its bytes and a TAB (none after the last chosen token); the
 * LF; both 30-bit headers recomputed.  Output records are dense and in file
 * order: header plus records is a valid .vcfc, and
 *   output == compress(decompress-samples / query-samples of the input)
 * whole bytes, for every accepted input.  The call stops with VCFC_E_FORMAT at
 * the first taken record that is not regular or not re-encodable, at a match
 * error, or where the LEN hops stop with 8 or more bytes left; the header and
 * the records before that point are kept (a valid shorter .vcfc).
 * VCFC_E_FORMAT with nothing written for a header the decoder refuses,
 * VCFC_E_ARG with nothing written for a bad column list (as above; also S ==
 * 0 with no list) or a bad region table.  Buffer variants: VCFC_E_NOSPACE if
 * out_cap is short (*out_len = size needed).  File variants create / truncate
 * out_vcfc before the input is parsed.
 * vcfc_extract_bound: an upper bound on the output of n_records records cut
 * to n_cols columns out of in_bytes of input (header included): in_bytes +
 * n_records * (n_cols + 1) -- a chosen class token costs at most one run byte
 * where it cost none of its own, any other chosen token its source bytes and
 * terminator plus one, and the source's last token has no terminator. */
uint64_t vcfc_extract_bound(uint64_t in_bytes, uint64_t n_records, uint64_t n_cols);
int vcfc_extract_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const uint32_t *cols, uint64_t n_cols,
                        int has_query, const char *ref, uint64_t ref_len, int has_range, uint64_t start, uint64_t end,
                        uint8_t *out, uint64_t out_cap, uint64_t *out_len);
int vcfc_extract_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_vcfc, const uint32_t *cols, uint64_t n_cols,
                      int has_query, const char *ref, uint64_t ref_len, int has_range, uint64_t start, uint64_t end);
int vcfc_extract_regions_buffer(vcfc_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const uint32_t *cols,
                                uint64_t n_cols, const uint8_t *table, uint64_t table_bytes, uint8_t *out,
                                uint64_t out_cap, uint64_t *out_len);
int vcfc_extract_regions_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_vcfc, const uint32_t *cols,
                              uint64_t n_cols, const uint8_t *table, uint64_t table_bytes);
/* Device-resident extract, exact in one call: the output records of records
 * d_in[d_rec_start[i], d_rec_start[i+1]) (d_select nullable: records with
 * d_select[i] == 0 are not taken and not checked) at d_out + d_rec_off[i];
 * d_rec_off[n] = total (n + 1 offsets).  `cols` as in
 * vcfc_decode_samples_device (NULL with n_cols == 0: all `samples` columns);
 * the same upload, synchronisation and 3 readable bytes past the last record.
 * A wave re-codes a record whose n_cols <= VCFC_EXTRACT_TILE_COLS (4096)
 * chosen columns fit its LDS tile; above that, and for records that are
 * regular but not simple (long or multi-token escapes, zero counts, an
 * LF-ended last token, more than 248 chosen other tokens), a byte-serial lane
 * does.  *d_err = ~0, or min over records of (i << 8 | 3): not regular, (i <<
 * 8 | 5): regular but not re-encodable (either way it and the records after it
 * have no meaningful output), (i << 8 | 0xFF): out_cap too small.
 * vcfc_extract_workspace_size takes the number of chosen columns (`samples`
 * where all are chosen). */
#define VCFC_EXTRACT_TILE_COLS 4096
uint64_t vcfc_extract_workspace_size(uint64_t n_records, uint64_t n_cols);
int vcfc_extract_samples_device(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_rec_start,
                                const uint8_t *d_select, uint64_t n, uint64_t samples, const uint32_t *cols,
                                uint64_t n_cols, uint8_t *d_out, uint64_t out_cap, uint64_t *d_rec_off, void *d_ws,
                                uint64_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- sparse layout: sparsify_file (reference src/sparse.cpp:290-580) -------
 * Record i of the .vcfc goes to data_start + (300e6 + POS_i) * 16384
 * (compute_sparse_offset, src/sparse.cpp:18-51) behind a 16-byte prefix
 * BE(dist_to_prev) BE(dist_to_next); the 8 bytes before data_start hold the
 * first record's offset in host byte order.  Output is a sparse file (holes
 * between records).  The GPU plans offsets and prefixes; the host writes. */
uint64_t vcfc_sparse_offset(uint64_t pos);
int vcfc_sparsify_file(vcfc_ctx *ctx, const char *in_vcfc, const char *out_sparse);
/* Sharded sparsify (multi-GPU, one process per GPU; SURVEY §8 e).  Rank
 * `rank` of `world` owns records [n*rank/world, n*(rank+1)/world) and plans
 * them on its GPU with one halo record on each side (the neighbours' offsets
 * give its first dist_to_prev and last dist_to_next).  info[4] =
 * {lo, hi, first unparsable record (global index, ~0 = none; bytes after the
 * last whole record count as record n), 1 if adjacent records of the planned
 * range overlap or are out of order}.
 * out_sparse == NULL: plan only.  Otherwise the slice is also written into
 * out_sparse (opened without truncation): rank 0 writes the header lines, the
 * owner of record 0 the first-offset slot.  Writing is only valid when every
 * rank's plan reported no error and no anomaly (records then occupy disjoint
 * ranges, so concurrent writes equal the reference's sequential ones);
 * otherwise one rank runs vcfc_sparsify_file, which replays the reference's
 * write order.  VCFC_E_ARG when asked to write a slice whose own plan is not
 * clean. */
int vcfc_sparsify_shard(vcfc_ctx *ctx, const char *in_vcfc, const char *out_sparse, int rank, int world,
                        uint64_t info[4]);
/* Sparse-file query: query_sparse_file_fd (reference src/main.cpp:235-582)
 * over a file written by sparsify, stdout-identical to the reference's
 * `main sparse-query`: start == end looks up the one slot of `start` and
 * writes its line unfiltered; otherwise the lines from the first record at or
 * after start's slot while CHROM equals `ref` and POS <= end (no filter at
 * all: the reference throws).  Lines go to out_fd as they are decoded (on the
 * GPU).  VCFC_E_FORMAT where the reference throws (every line it writes
 * before is written); VCFC_E_IO when the file does not open. */
int vcfc_sparse_query_file(vcfc_ctx *ctx, const char *in_sparse, const char *ref, uint64_t ref_len, int has_range,
                           uint64_t start, uint64_t end, int out_fd);

/* Device plan: records d_recs[d_rec_off[i] .. d_rec_off[i+1]); outputs
 * d_file_off[i] and d_prefix16[16 i ..]; d_status[0] = ~0 or (row << 8 |
 * VCFC_E_FORMAT) of the first record whose POS does not parse, d_status[1] =
 * 1 if records overlap / are out of order (write them in order). */
int vcfc_sparse_plan_device(const uint8_t *d_recs, const uint64_t *d_rec_off, uint64_t n, uint64_t data_start,
                            uint64_t *d_file_off, uint8_t *d_prefix16, uint64_t *d_status, void *stream);

/* ---- device-side helpers used by the benchmark ---------------------------
 * Synthetic genotype rows generated in HBM (no host round trip).  `law`:
 *   0 = random_vcf law (alleles i.i.d. 0/1/2 with p .90/.08/.02,
 *       reference other/random_vcf.py:66-70)
 *   1 = chr22-shaped (per-row alt-allele frequency from d_row_af; ~1% of
 *       rows multi-allelic)
 *   2 = general shapes (d_row_af = kind + allele frequency: haploid,
 *       GT:DP:GQ, missing, unphased; vcf-compression_amd/workload.py)
 *   3 = alternating classes, the RLE worst case (d_row_af = kind: 0 = the
 *       classes 0|0 0|1 1|0 1|1 cycling, every token a new run; 1 = alleles
 *       i.i.d. at frequency 1/2)
 * The prefix (9 columns + '\t') of row i is copied from
 * d_prefix[d_prefix_off[i] .. d_prefix_off[i+1]); row i is written at
 * d_buf + d_line_off[i] with S tokens and a trailing '\n'. */
int vcfc_synth_rows_device(uint8_t *d_buf, const uint64_t *d_line_off, uint64_t n,
                           const uint8_t *d_prefix, const uint64_t *d_prefix_off,
                           const float *d_row_af, uint32_t samples, int law, uint64_t seed,
                           void *stream);
/* The same rows as rows [row_base, row_base + n) of a batch generated whole
 * with this seed (the genotypes hash the batch row index): a rank generates
 * its slice of one fixed dataset (bench.py's strong split). */
int vcfc_synth_rows_device_at(uint8_t *d_buf, const uint64_t *d_line_off, uint64_t n,
                              const uint8_t *d_prefix, const uint64_t *d_prefix_off,
                              const float *d_row_af, uint32_t samples, int law, uint64_t seed,
                              uint64_t row_base, void *stream);

/* Per-record 64-bit digests of an encoded batch, in place on the GPU:
 * d_hash[i] = digest of d_recs[d_rec_off[i] .. d_rec_off[i+1]).  Digest:
 * h = len * 0x9E3779B97F4A7C15 + sum_k mix(w_k ^ (k * 0xD1B54A32D192ED03 +
 * 0x8CB92BA72F3D8DD7)) mod 2^64, result mix(h); w_k = bytes [8k, 8k+8)
 * little-endian, zero-padded; mix = splitmix64's finaliser.  Lets a caller
 * verify multi-GB batches against a CPU encode by comparing 8 B per row (no
 * reference counterpart).  Enqueued on `stream`. */
int vcfc_record_hash_device(const uint8_t *d_recs, const uint64_t *d_rec_off, uint64_t n, uint64_t *d_hash,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif
