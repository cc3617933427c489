"""Python binding (ctypes) of libvcfc.so -- the C ABI in include/vcfc.h.

Mirrors the reference's operator interface for the encode path:
  compress_data_line(line, add_newline=True)   (reference src/compress.hpp:20-23)
  compress_file(in_path, out_path)             (reference src/compress.cpp:205-257)
  decompress / decompress_file                 (reference src/compress.cpp:1214-1257)
  parse_coordinate_string, query / query_file  (reference src/main.cpp:3777-4026)
  create_binned_index / query_binned_index     (reference src/main.cpp:1284-1637, 2974-3349)
  create_sparse_index / query_sparse_index     (reference src/main.cpp:854-999, 1002-1281)
  gap_analysis                                 (reference src/main.cpp:3931-3980)
Errors raise VcfValidationError / RuntimeError like the reference's exceptions
(src/utils.hpp:117-123, src/compress.cpp:9-11,231-234).

There is no CPU fallback: without a visible gfx950 GPU, Context() raises.
If PyTorch is used in the same process, import torch BEFORE loading this
module so both share one HIP runtime (libvcfc.so binds to whatever
libamdhip64.so is already loaded).
"""
import collections
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("VCFC_LIB") or os.path.join(ROOT, "build", "libvcfc.so")

OK, E_LT8COLS, E_8COLS, E_HEADER, E_NOSPACE, E_ARG, E_HIP, E_IO, E_FORMAT = range(9)
E_TOOLONG = 10   # a data line longer than MAX_LINE (include/vcfc.h VCFC_E_TOOLONG)
MAX_LINE = (1 << 29) - 64
NO_ERROR = (1 << 64) - 1

EXPORTS = [
    "vcfc_version", "vcfc_strerror", "vcfc_ctx_create", "vcfc_ctx_destroy",
    "vcfc_compress_data_line", "vcfc_encode_bound", "vcfc_encode_workspace_size",
    "vcfc_encode_rows_device", "vcfc_encode_rows", "vcfc_compress_file",
    "vcfc_compress_bound", "vcfc_compress_buffer", "vcfc_synth_rows_device", "vcfc_synth_rows_device_at",
    "vcfc_timer_create", "vcfc_timer_destroy", "vcfc_encode_rows_device_timed", "vcfc_timer_read",
    "vcfc_sparse_offset", "vcfc_sparsify_file", "vcfc_sparse_plan_device",
    "vcfc_decompress_buffer", "vcfc_decompress_file", "vcfc_decode_workspace_size",
    "vcfc_decode_records_device", "vcfc_parse_query", "vcfc_query_buffer", "vcfc_query_file",
    "vcfc_query_match_device", "vcfc_decode_selected_device", "vcfc_sparse_query_file",
    "vcfc_sparsify_shard", "vcfc_ctx_set_ingest_chunk", "vcfc_record_hash_device",
    "vcfc_compress_range", "vcfc_compress_device", "vcfc_compress_range_held", "vcfc_held_place",
    "vcfc_held_sizes", "vcfc_held_free", "vcfc_ctx_set_line_index", "vcfc_ctx_set_trace",
    "vcfc_ctx_set_deferred_records", "vcfc_encode_deferred_rows",
    "vcfc_index_workspace_size", "vcfc_binned_index_device", "vcfc_record_span_device",
    "vcfc_create_binned_index_buffer", "vcfc_create_binned_index_file",
    "vcfc_query_binned_index_buffer", "vcfc_query_binned_index_file",
    "vcfc_sparse_index_workspace_size", "vcfc_sparse_index_offset", "vcfc_sparse_index_device",
    "vcfc_create_sparse_index_file", "vcfc_query_sparse_index_file",
    "vcfc_decode_sizes_workspace_size", "vcfc_decode_sizes_device", "vcfc_gap_analysis_file",
    "vcfc_sample_columns", "vcfc_subset_workspace_size", "vcfc_decode_samples_device",
    "vcfc_decompress_samples_buffer", "vcfc_decompress_samples_file",
    "vcfc_query_samples_buffer", "vcfc_query_samples_file",
    "vcfc_counts_workspace_size", "vcfc_counts_lds_samples", "vcfc_counts_trip_records", "vcfc_genotype_counts_device",
    "vcfc_genotype_counts_buffer", "vcfc_genotype_counts_file",
    "vcfc_regions_build", "vcfc_regions_workspace_size", "vcfc_regions_upload", "vcfc_regions_match_device",
    "vcfc_query_regions_buffer", "vcfc_query_regions_file",
    "vcfc_query_samples_regions_buffer", "vcfc_query_samples_regions_file",
    "vcfc_genotype_counts_regions_buffer", "vcfc_genotype_counts_regions_file",
    "vcfc_matrix_row_bytes", "vcfc_matrix_lds_samples", "vcfc_matrix_trip_records", "vcfc_matrix_workspace_size",
    "vcfc_genotype_matrix_device",
    "vcfc_genotype_matrix_buffer", "vcfc_genotype_matrix_regions_buffer", "vcfc_export_bed_file",
    "vcfc_export_bed_regions_file",
    "vcfc_ld_workspace_size", "vcfc_ld_tables_device", "vcfc_ld_window_device", "vcfc_ld_window_buffer",
    "vcfc_ld_window_regions_buffer", "vcfc_ld_window_file", "vcfc_ld_window_regions_file",
    "vcfc_kin_workspace_size", "vcfc_kin_tables_device", "vcfc_kin_records_device", "vcfc_kinship_buffer",
    "vcfc_kinship_regions_buffer", "vcfc_kinship_file", "vcfc_kinship_regions_file",
    "vcfc_extract_bound", "vcfc_extract_workspace_size", "vcfc_extract_samples_device", "vcfc_extract_buffer",
    "vcfc_extract_file", "vcfc_extract_regions_buffer", "vcfc_extract_regions_file",
]
LINE_INDEX_HOP, LINE_INDEX_SCAN = 0, 1                       # include/vcfc.h VCFC_LINE_INDEX_*
TRACE_INGEST, TRACE_DEVICE, TRACE_SPARSE_QUERY = 1, 2, 4     # include/vcfc.h VCFC_TRACE_*
TRACE_INDEX = 8
INDEX_ENTRY_BYTES = 13                                       # include/vcfc.h VCFC_INDEX_ENTRY_BYTES


class VcfValidationError(RuntimeError):
    """Same meaning as the reference's VcfValidationError (src/utils.hpp:117-123)."""


class LengthError(RuntimeError):
    """The reference aborts with std::length_error on 8-column data lines."""


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libvcfc.so not built: run `make -C vcf-compression_amd` (or __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    vp, u64, u32, i64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
    L.vcfc_version.restype = ctypes.c_char_p
    L.vcfc_strerror.restype = ctypes.c_char_p
    L.vcfc_strerror.argtypes = [ctypes.c_int]
    L.vcfc_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.vcfc_ctx_destroy.argtypes = [vp]
    L.vcfc_ctx_destroy.restype = None
    L.vcfc_ctx_set_ingest_chunk.argtypes = [vp, u64]
    # Exports added since round 3 are bound only when present: A/B runs load
    # older builds of the library (tools/ab.sh, VCFC_LIB); calling one that
    # the loaded build lacks raises a clear error (_need).  test_capi checks
    # that the current build exports every one of them.
    late = {"vcfc_ctx_set_line_index": [vp, ctypes.c_int], "vcfc_ctx_set_trace": [vp, ctypes.c_uint],
            "vcfc_ctx_set_deferred_records": [vp, ctypes.c_int],
            "vcfc_encode_deferred_rows": [vp, u64, u64, vp, ctypes.POINTER(u64)],
            # the binned external index
            "vcfc_index_workspace_size": [u64],
            "vcfc_binned_index_device": [vp, vp, u64, u64, u64, vp, u64, vp, vp, vp, u64, vp, vp],
            "vcfc_record_span_device": [vp, vp, u64, vp, vp, vp, vp, vp],
            "vcfc_create_binned_index_buffer": [vp, vp, u64, u64, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(i64)],
            "vcfc_create_binned_index_file": [vp, ctypes.c_char_p, ctypes.c_char_p, u64],
            "vcfc_query_binned_index_buffer": [vp, vp, u64, vp, u64, ctypes.c_char_p, u64, ctypes.c_int, u64, u64, vp,
                                               u64, ctypes.POINTER(u64)],
            "vcfc_query_binned_index_file": [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, u64, ctypes.c_int,
                                             u64, u64, ctypes.c_int],
            # the sparse external index and gap-analysis
            "vcfc_sparse_index_workspace_size": [u64],
            "vcfc_sparse_index_offset": [u64],
            "vcfc_sparse_index_device": [vp, vp, u64, u64, vp, vp, vp, vp, vp, u64, vp, vp],
            "vcfc_create_sparse_index_file": [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(i64),
                                              ctypes.POINTER(ctypes.c_int)],
            "vcfc_query_sparse_index_file": [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, u64, ctypes.c_int,
                                             u64, u64, ctypes.c_int],
            "vcfc_decode_sizes_workspace_size": [u64],
            "vcfc_decode_sizes_device": [vp, u64, vp, u64, u64, vp, vp, vp, vp, vp, u64, vp, vp],
            "vcfc_gap_analysis_file": [vp, ctypes.c_char_p, ctypes.c_char_p],
            # the sample subset
            "vcfc_sample_columns": [vp, u64, ctypes.c_char_p, u64, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)],
            "vcfc_subset_workspace_size": [u64, u64],
            "vcfc_decode_samples_device": [vp, u64, vp, vp, u64, u64, vp, u64, vp, u64, vp, vp, u64, vp, vp],
            "vcfc_decompress_samples_buffer": [vp, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64)],
            "vcfc_decompress_samples_file": [vp, ctypes.c_char_p, ctypes.c_char_p, vp, u64],
            "vcfc_query_samples_buffer": [vp, vp, u64, ctypes.c_char_p, u64, ctypes.c_int, u64, u64, vp, u64, vp, u64,
                                          ctypes.POINTER(u64)],
            "vcfc_query_samples_file": [vp, ctypes.c_char_p, ctypes.c_char_p, u64, ctypes.c_int, u64, u64, vp, u64,
                                        ctypes.c_int],
            # genotype counts
            "vcfc_counts_workspace_size": [u64, u64],
            "vcfc_counts_lds_samples": [],
            "vcfc_counts_trip_records": [u64, ctypes.c_int],
            "vcfc_genotype_counts_device": [vp, u64, vp, vp, u64, u64, vp, vp, vp, u64, vp, vp],
            "vcfc_genotype_counts_buffer": [vp, vp, u64, ctypes.c_int, ctypes.c_char_p, u64, ctypes.c_int, u64, u64, vp,
                                            vp, u64, ctypes.POINTER(u64), vp, u64, ctypes.POINTER(u64),
                                            ctypes.POINTER(u64)],
            "vcfc_genotype_counts_file": [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
                                          ctypes.c_char_p, u64, ctypes.c_int, u64, u64],
            # region lists
            "vcfc_regions_build": [ctypes.c_char_p, u64, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                   ctypes.POINTER(u64)],
            "vcfc_regions_workspace_size": [u64],
            "vcfc_regions_upload": [vp, u64, vp, u64, vp],
            "vcfc_regions_match_device": [vp, vp, u64, vp, u64, vp, vp, vp],
            "vcfc_query_regions_buffer": [vp, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64)],
            "vcfc_query_regions_file": [vp, ctypes.c_char_p, vp, u64, ctypes.c_int],
            "vcfc_query_samples_regions_buffer": [vp, vp, u64, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64)],
            "vcfc_query_samples_regions_file": [vp, ctypes.c_char_p, vp, u64, vp, u64, ctypes.c_int],
            "vcfc_genotype_counts_regions_buffer": [vp, vp, u64, vp, u64, vp, vp, u64, ctypes.POINTER(u64), vp, u64,
                                                    ctypes.POINTER(u64), ctypes.POINTER(u64)],
            "vcfc_genotype_counts_regions_file": [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, vp, u64],
            # the genotype matrix
            "vcfc_matrix_row_bytes": [ctypes.c_int, u64],
            "vcfc_matrix_lds_samples": [ctypes.c_int],
            "vcfc_matrix_trip_records": [ctypes.c_int],
            "vcfc_matrix_workspace_size": [u64, u64, ctypes.c_int],
            "vcfc_genotype_matrix_device": [vp, u64, vp, vp, u64, u64, ctypes.c_int, vp, u64, u64, vp, vp, u64, vp, vp],
            "vcfc_genotype_matrix_buffer": [vp, vp, u64, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, u64, ctypes.c_int,
                                            u64, u64, vp, u64, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                            ctypes.POINTER(u64)],
            "vcfc_genotype_matrix_regions_buffer": [vp, vp, u64, ctypes.c_int, vp, u64, vp, u64, vp, u64,
                                                    ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)],
            "vcfc_export_bed_file": [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, u64,
                                     ctypes.c_int, u64, u64],
            "vcfc_export_bed_regions_file": [vp, ctypes.c_char_p, ctypes.c_char_p, vp, u64],
            # the LD window
            "vcfc_ld_workspace_size": [u64, u64, u64],
            "vcfc_ld_tables_device": [vp, u64, u64, u64, u64, vp, u64, vp, u64, vp, vp],
            "vcfc_ld_window_device": [vp, u64, vp, vp, u64, u64, u64, vp, u64, vp, vp, u64, vp, vp],
            "vcfc_ld_window_buffer": [vp, vp, u64, u64, ctypes.c_int, ctypes.c_char_p, u64, ctypes.c_int, u64, u64, vp, u64,
                                      vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)],
            "vcfc_ld_window_regions_buffer": [vp, vp, u64, u64, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64),
                                              ctypes.POINTER(u64)],
            "vcfc_ld_window_file": [vp, ctypes.c_char_p, ctypes.c_char_p, u64, ctypes.c_double, ctypes.c_int,
                                    ctypes.c_char_p, u64, ctypes.c_int, u64, u64],
            "vcfc_ld_window_regions_file": [vp, ctypes.c_char_p, ctypes.c_char_p, u64, ctypes.c_double, vp, u64],
            # kinship
            "vcfc_kin_workspace_size": [u64, u64],
            "vcfc_kin_tables_device": [vp, u64, u64, u64, vp, u64, ctypes.c_int, vp, u64, vp, vp],
            "vcfc_kin_records_device": [vp, u64, vp, vp, u64, u64, vp, u64, ctypes.c_int, vp, vp, u64, vp, vp],
            "vcfc_kinship_buffer": [vp, vp, u64, ctypes.c_int, ctypes.c_char_p, u64, ctypes.c_int, u64, u64, vp, u64, vp, u64,
                                    ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)],
            "vcfc_kinship_regions_buffer": [vp, vp, u64, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64),
                                            ctypes.POINTER(u64), ctypes.POINTER(u64)],
            "vcfc_kinship_file": [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                  ctypes.c_char_p, u64, ctypes.c_int, u64, u64],
            "vcfc_kinship_regions_file": [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_double, vp, u64],
            # extract
            "vcfc_extract_bound": [u64, u64, u64],
            "vcfc_extract_workspace_size": [u64, u64],
            "vcfc_extract_samples_device": [vp, u64, vp, vp, u64, u64, vp, u64, vp, u64, vp, vp, u64, vp, vp],
            "vcfc_extract_buffer": [vp, vp, u64, vp, u64, ctypes.c_int, ctypes.c_char_p, u64, ctypes.c_int, u64, u64, vp,
                                    u64, ctypes.POINTER(u64)],
            "vcfc_extract_file": [vp, ctypes.c_char_p, ctypes.c_char_p, vp, u64, ctypes.c_int, ctypes.c_char_p, u64,
                                  ctypes.c_int, u64, u64],
            "vcfc_extract_regions_buffer": [vp, vp, u64, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64)],
            "vcfc_extract_regions_file": [vp, ctypes.c_char_p, ctypes.c_char_p, vp, u64, vp, u64]}
    for name, args in late.items():
        if hasattr(L, name):
            getattr(L, name).argtypes = args
    for name in ("vcfc_index_workspace_size", "vcfc_sparse_index_workspace_size", "vcfc_sparse_index_offset",
                 "vcfc_decode_sizes_workspace_size", "vcfc_subset_workspace_size", "vcfc_counts_workspace_size",
                 "vcfc_counts_lds_samples", "vcfc_regions_workspace_size", "vcfc_matrix_row_bytes",
                 "vcfc_matrix_lds_samples", "vcfc_matrix_workspace_size", "vcfc_extract_bound",
                 "vcfc_extract_workspace_size", "vcfc_counts_trip_records", "vcfc_matrix_trip_records",
                 "vcfc_ld_workspace_size", "vcfc_kin_workspace_size"):
        if hasattr(L, name):
            getattr(L, name).restype = u64
    L.vcfc_record_hash_device.argtypes = [vp, vp, u64, vp, vp]
    L.vcfc_compress_range.argtypes = [vp, ctypes.c_char_p, u64, u64, ctypes.c_int, u64, ctypes.POINTER(u64),
                                      ctypes.POINTER(i64), ctypes.POINTER(u64)]
    L.vcfc_compress_range_held.argtypes = [vp, ctypes.c_char_p, u64, u64, u64, ctypes.c_char_p, ctypes.POINTER(vp),
                                           ctypes.POINTER(u64), ctypes.POINTER(i64), ctypes.POINTER(u64)]
    L.vcfc_held_place.argtypes = [vp, ctypes.c_int, u64]
    L.vcfc_held_sizes.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.vcfc_held_sizes.restype = None
    L.vcfc_held_free.argtypes = [vp]
    L.vcfc_held_free.restype = None
    L.vcfc_compress_data_line.argtypes = [vp, ctypes.c_char_p, u64, ctypes.c_int, vp, u64, ctypes.POINTER(u64)]
    L.vcfc_encode_bound.restype = u64
    L.vcfc_encode_bound.argtypes = [u64, u64]
    L.vcfc_encode_workspace_size.restype = u64
    L.vcfc_encode_workspace_size.argtypes = [u64, u64]
    L.vcfc_encode_rows_device.argtypes = [vp, vp, vp, u64, u64, vp, u64, vp, vp, u64, vp, vp]
    L.vcfc_encode_rows.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, vp, ctypes.POINTER(i64)]
    L.vcfc_compress_file.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(i64)]
    L.vcfc_compress_bound.restype = u64
    L.vcfc_compress_bound.argtypes = [u64]
    L.vcfc_compress_buffer.argtypes = [vp, vp, u64, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(i64)]
    L.vcfc_compress_device.argtypes = [vp, vp, u64, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(i64)]
    L.vcfc_timer_create.argtypes = [ctypes.POINTER(vp)]
    L.vcfc_timer_destroy.argtypes = [vp]
    L.vcfc_timer_destroy.restype = None
    L.vcfc_encode_rows_device_timed.argtypes = [vp, vp, vp, u64, u64, vp, u64, vp, vp, u64, vp, vp, vp]
    L.vcfc_timer_read.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64)]
    L.vcfc_sparse_offset.restype = u64
    L.vcfc_sparse_offset.argtypes = [u64]
    L.vcfc_sparsify_file.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p]
    L.vcfc_sparsify_shard.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(u64)]
    L.vcfc_sparse_plan_device.argtypes = [vp, vp, u64, u64, vp, vp, vp, vp]
    L.vcfc_decompress_buffer.argtypes = [vp, vp, u64, vp, u64, ctypes.POINTER(u64)]
    L.vcfc_decompress_file.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p]
    L.vcfc_decode_workspace_size.restype = u64
    L.vcfc_decode_workspace_size.argtypes = [u64]
    L.vcfc_decode_records_device.argtypes = [vp, u64, vp, u64, u64, vp, u64, vp, vp, u64, vp, ctypes.c_int, vp]
    L.vcfc_synth_rows_device.argtypes = [vp, vp, u64, vp, vp, vp, u32, ctypes.c_int, u64, vp]
    L.vcfc_synth_rows_device_at.argtypes = [vp, vp, u64, vp, vp, vp, u32, ctypes.c_int, u64, u64, vp]
    pu64 = ctypes.POINTER(u64)
    L.vcfc_parse_query.argtypes = [ctypes.c_char_p, u64, pu64, ctypes.POINTER(ctypes.c_int), pu64, pu64]
    L.vcfc_query_buffer.argtypes = [vp, vp, u64, ctypes.c_char_p, u64, ctypes.c_int, u64, u64, vp, u64, pu64]
    L.vcfc_query_file.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, u64, ctypes.c_int, u64, u64, ctypes.c_int]
    L.vcfc_decode_selected_device.argtypes = [vp, u64, vp, vp, u64, u64, vp, u64, vp, vp, u64, vp, ctypes.c_int, vp]
    L.vcfc_query_match_device.argtypes = [vp, vp, u64, vp, u64, ctypes.c_int, u64, u64, vp, vp, vp]
    L.vcfc_sparse_query_file.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, u64, ctypes.c_int, u64, u64,
                                         ctypes.c_int]
    _lib = L
    return L


def strerror(st):
    return lib().vcfc_strerror(st).decode()


def raise_for(st, where=""):
    if st == OK:
        return
    msg = strerror(st) + (" (%s)" % where if where else "")
    if st in (E_LT8COLS, E_HEADER):
        raise VcfValidationError(msg)
    if st == E_8COLS:
        raise LengthError(msg)
    raise RuntimeError(msg)


class VcfCoordinateQuery(collections.namedtuple("VcfCoordinateQuery", "reference_name has_range start end")):
    """VcfCoordinateQuery (reference src/main.cpp:60-90): a reference name
    (b"" matches any) and, when has_range, an inclusive POS range."""


def parse_coordinate_string(q):
    """parse_coordinate_string (reference src/main.cpp:3993-4026), through
    the C ABI.  Raises ValueError with the reference's message where it
    prints one and returns -1."""
    qb = q.encode() if isinstance(q, str) else bytes(q)
    ref_len, has_range, start, end = ctypes.c_uint64(), ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
    st = lib().vcfc_parse_query(qb, len(qb), ctypes.byref(ref_len), ctypes.byref(has_range), ctypes.byref(start),
                                ctypes.byref(end))
    if st != 0:
        colon = qb.find(b":")
        dash = qb.find(b"-", colon + 1)
        msg = {1: "Query must contain a dash character: <ref>:<start>-<end>",
               2: "Failed to parse int from start position: %s" % qb[colon + 1:dash].decode(errors="replace"),
               3: "Failed to parse int from end position: %s" % qb[dash + 1:].decode(errors="replace")}.get(st)
        raise ValueError(msg or strerror(st))
    return VcfCoordinateQuery(qb[:ref_len.value], bool(has_range.value), start.value, end.value)


HOLD_CAP_DEFAULT = 32 << 30     # VCFC_HOLD_GB unset: at most 32 GiB held per rank
INGEST_PINNED_BYTES = 1 << 30   # a rank's own pinned ingest slots and staging (3 x 128 MiB + margin)


def mem_available(meminfo="/proc/meminfo"):
    """MemAvailable of this host in bytes (None when it cannot be read)."""
    try:
        with open(meminfo) as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) * 1024
    except OSError:
        pass
    return None


def hold_bytes(local_world=None, avail=None):
    """How much output one rank may hold in host memory before it spills
    (Context.compress_range_held's mem_bound): a share of the host's available
    memory -- 3/4 of MemAvailable split over the node's ranks, less each rank's
    pinned ingest buffers -- capped by VCFC_HOLD_GB (default 32 GiB), and at
    least 64 MiB (one hold block).  Bounding by the host, not a constant,
    keeps 8 ranks from overcommitting a node into the OOM killer while their
    peers wait in the all-gather."""
    import os
    if local_world is None:
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")) or 1)
    env = os.environ.get("VCFC_HOLD_GB")
    cap = int(float(env) * (1 << 30)) if env else HOLD_CAP_DEFAULT
    avail = mem_available() if avail is None else avail
    if avail is not None:
        cap = min(cap, (avail * 3 // 4) // max(1, local_world) - INGEST_PINNED_BYTES)
    return max(64 << 20, cap)


class Held:
    """Output of Context.compress_range_held, placed once its offset is known.
    Owns host memory (up to its bound) and a spill file: free() releases them,
    as do `with` and garbage collection."""

    def __init__(self, h):
        self._h = h

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def place(self, fd, off):
        """Write every held byte at file offset `off` of fd; returns the status."""
        return lib().vcfc_held_place(self._h, fd, off) if self._h else E_ARG

    def sizes(self):
        m, sp = ctypes.c_uint64(0), ctypes.c_uint64(0)
        lib().vcfc_held_sizes(self._h, ctypes.byref(m), ctypes.byref(sp))
        return m.value, sp.value

    def free(self):
        if self._h:
            lib().vcfc_held_free(self._h)
            self._h = None


class Context:
    """One GPU (device ordinal).  Raises if no GPU is visible."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        st = lib().vcfc_ctx_create(device, ctypes.byref(self._h))
        if st != OK:
            raise RuntimeError("vcfc: cannot create a GPU context: " + strerror(st))

    def close(self):
        if self._h:
            lib().vcfc_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_ingest_chunk(self, chunk_bytes):
        """Input chunk of compress_file / compress_buffer (0 = default 128 MiB);
        the output does not depend on it."""
        raise_for(lib().vcfc_ctx_set_ingest_chunk(self._h, int(chunk_bytes)))

    def set_line_index(self, mode):
        """compress_device's line index: "hop" (default; guessed line ends,
        checked) or "scan" (every byte).  The output does not depend on it."""
        raise_for(_need("vcfc_ctx_set_line_index")(self._h, {"hop": LINE_INDEX_HOP, "scan": LINE_INDEX_SCAN}[mode]))

    def set_deferred_records(self, on):
        """Deferred records for the file / device compress calls (on by
        default since round 5): rows whose first genotype chunk is all
        escapes are sized first and written straight into the output
        (include/vcfc.h).  The output does not depend on it."""
        raise_for(_need("vcfc_ctx_set_deferred_records")(self._h, 1 if on else 0))

    def set_trace(self, flags):
        """Stage timings of the host drivers to stderr (TRACE_* flags)."""
        raise_for(_need("vcfc_ctx_set_trace")(self._h, int(flags)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- reference interface ------------------------------------------------
    def compress_data_line(self, line, add_newline=True):
        """bytes line (no '\\n') -> record bytes, as compress_data_line."""
        cap = lib().vcfc_encode_bound(1, len(line)) + 16
        buf = ctypes.create_string_buffer(cap)
        n = ctypes.c_uint64(0)
        st = lib().vcfc_compress_data_line(self._h, line, len(line), int(add_newline), buf, cap, ctypes.byref(n))
        raise_for(st)
        return buf.raw[:n.value]

    def compress_buffer(self, data):
        """Whole VCF (bytes) -> .vcfc bytes, as compress()."""
        cap = lib().vcfc_compress_bound(len(data))
        out = np.empty(cap, dtype=np.uint8)
        n = ctypes.c_uint64(0)
        line = ctypes.c_int64(-1)
        src = np.frombuffer(data, dtype=np.uint8)
        st = lib().vcfc_compress_buffer(self._h, src.ctypes.data, len(data), out.ctypes.data, cap,
                                        ctypes.byref(n), ctypes.byref(line))
        raise_for(st, "line %d" % line.value)
        return out[:n.value].tobytes()

    def compress_device(self, d_in, n, d_out, out_cap):
        """compress() over file bytes in device memory (pointers): d_in[0, n)
        -> d_out; returns (status, out_len, err_line) without raising."""
        k = ctypes.c_uint64(0)
        line = ctypes.c_int64(-1)
        st = lib().vcfc_compress_device(self._h, d_in, n, d_out, out_cap, ctypes.byref(k), ctypes.byref(line))
        return st, k.value, line.value

    def compress_status(self, data):
        """Like compress_buffer without raising: (status, bytes, err_line).
        On a failing line the bytes are everything the reference writes
        before it throws; err_line is its 1-based line number."""
        cap = lib().vcfc_compress_bound(len(data))
        out = np.empty(cap, dtype=np.uint8)
        n = ctypes.c_uint64(0)
        line = ctypes.c_int64(-1)
        src = np.frombuffer(data, dtype=np.uint8)
        st = lib().vcfc_compress_buffer(self._h, src.ctypes.data, len(data), out.ctypes.data, cap,
                                        ctypes.byref(n), ctypes.byref(line))
        return st, out[:n.value].tobytes(), line.value

    def compress_file(self, in_path, out_path):
        line = ctypes.c_int64(-1)
        st = lib().vcfc_compress_file(self._h, in_path.encode(), out_path.encode(), ctypes.byref(line))
        raise_for(st, "line %d" % line.value)

    def compress_range(self, in_path, off, length, out_fd, out_off=0):
        """One shard of a sharded compress: bytes [off, off + length) of
        in_path (whole lines) -> out_fd at out_off.  Returns (status,
        bytes written, 1-based failing line in the range or -1, lines in the
        range); does not raise (ranks exchange statuses first)."""
        nb, line, lines = ctypes.c_uint64(0), ctypes.c_int64(-1), ctypes.c_uint64(0)
        st = lib().vcfc_compress_range(self._h, in_path.encode(), off, length, out_fd, out_off, ctypes.byref(nb),
                                       ctypes.byref(line), ctypes.byref(lines))
        return st, nb.value, line.value, lines.value

    def compress_range_held(self, in_path, off, length, mem_bound=None, spill_dir=None):
        """compress_range with the output held (host memory up to mem_bound
        bytes -- default hold_bytes(), this rank's share of the host -- the
        rest in a spill file) until its file offset is known.
        Returns (status, bytes, failing line in the range or -1, lines in the
        range, Held); does not raise."""
        if mem_bound is None:
            mem_bound = hold_bytes()
        nb, line, lines, h = ctypes.c_uint64(0), ctypes.c_int64(-1), ctypes.c_uint64(0), ctypes.c_void_p()
        st = lib().vcfc_compress_range_held(self._h, in_path.encode(), off, length, mem_bound,
                                            spill_dir.encode() if spill_dir else None, ctypes.byref(h),
                                            ctypes.byref(nb), ctypes.byref(line), ctypes.byref(lines))
        return st, nb.value, line.value, lines.value, Held(h.value)

    def decompress_buffer(self, data, cap=None):
        """.vcfc bytes -> VCF bytes, as decompress2_fd (reference
        src/compress.cpp:1214-1257).  Returns (status, bytes): on
        VCFC_E_FORMAT the bytes are what the reference writes before it
        throws."""
        src = np.frombuffer(data, dtype=np.uint8)
        cap = cap if cap is not None else 16 * len(data) + 4096
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint8)
            n = ctypes.c_uint64(0)
            st = lib().vcfc_decompress_buffer(self._h, src.ctypes.data, len(data), out.ctypes.data, cap,
                                              ctypes.byref(n))
            if st == E_NOSPACE and n.value > cap:
                cap = n.value
                continue
            return st, out[:n.value].tobytes()

    def decompress(self, data):
        """Like decompress_buffer, raising where the reference throws."""
        st, out = self.decompress_buffer(data)
        raise_for(st)
        return out

    def decompress_file(self, in_path, out_path):
        raise_for(lib().vcfc_decompress_file(self._h, in_path.encode(), out_path.encode()))

    def query_buffer(self, data, query, cap=None):
        """query_compressed_file (reference src/main.cpp:3777-3929) over .vcfc
        bytes: the matching lines (no header).  `query` is a
        VcfCoordinateQuery or a coordinate string.  Returns (status, bytes):
        on VCFC_E_FORMAT the bytes are every line the reference writes before
        it throws."""
        if not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        src = np.frombuffer(data, dtype=np.uint8)
        cap = cap if cap is not None else 16 * len(data) + 4096
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint8)
            n = ctypes.c_uint64(0)
            st = lib().vcfc_query_buffer(self._h, src.ctypes.data, len(data), query.reference_name,
                                         len(query.reference_name), int(query.has_range), query.start, query.end,
                                         out.ctypes.data, cap, ctypes.byref(n))
            if st == E_NOSPACE and n.value > cap:
                cap = n.value
                continue
            return st, out[:n.value].tobytes()

    def query(self, data, query):
        """Like query_buffer, raising where the reference throws."""
        st, out = self.query_buffer(data, query)
        raise_for(st)
        return out

    def query_file(self, in_path, query, out_fd=1):
        """Matching lines of a .vcfc file written to out_fd (stdout by
        default), as `main query <file> <query>`."""
        if not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        raise_for(lib().vcfc_query_file(self._h, in_path.encode(), query.reference_name, len(query.reference_name),
                                        int(query.has_range), query.start, query.end, out_fd))

    def decompress_samples_buffer(self, data, cols, cap=None):
        """decompress-samples: the header and every line cut
        to the 0-based sample columns `cols`, in that order.  Returns (status,
        bytes): on VCFC_E_FORMAT the bytes are the header and the lines before
        the first record that is not regular; VCFC_E_ARG (no column, a column
        past the header's samples, a column listed twice) writes nothing."""
        src = np.frombuffer(data, dtype=np.uint8)
        c = np.asarray(cols, dtype=np.uint32)
        cap = cap if cap is not None else len(data) + 16 * len(c) * (len(data) // 64 + 1) + 4096
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint8)
            n = ctypes.c_uint64(0)
            st = _need("vcfc_decompress_samples_buffer")(self._h, src.ctypes.data, len(data), c.ctypes.data, len(c),
                                                         out.ctypes.data, cap, ctypes.byref(n))
            if st == E_NOSPACE and n.value > cap:
                cap = n.value
                continue
            return st, out[:n.value].tobytes()

    def decompress_samples_file(self, in_path, out_path, cols):
        c = np.asarray(cols, dtype=np.uint32)
        raise_for(_need("vcfc_decompress_samples_file")(self._h, in_path.encode(), out_path.encode(), c.ctypes.data,
                                                        len(c)))

    def query_samples_buffer(self, data, query, cols, cap=None):
        """query-samples: the matching lines (no header) cut to `cols`.
        Records match as in query_buffer; only matching records must be
        regular.  Returns (status, bytes)."""
        if not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        src = np.frombuffer(data, dtype=np.uint8)
        c = np.asarray(cols, dtype=np.uint32)
        cap = cap if cap is not None else len(data) + 16 * len(c) * (len(data) // 64 + 1) + 4096
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint8)
            n = ctypes.c_uint64(0)
            st = _need("vcfc_query_samples_buffer")(self._h, src.ctypes.data, len(data), query.reference_name,
                                                    len(query.reference_name), int(query.has_range), query.start,
                                                    query.end, c.ctypes.data, len(c), out.ctypes.data, cap,
                                                    ctypes.byref(n))
            if st == E_NOSPACE and n.value > cap:
                cap = n.value
                continue
            return st, out[:n.value].tobytes()

    def query_samples_file(self, in_path, query, cols, out_fd=1):
        """As `main query-samples <file> <query> <names>`, with columns."""
        if not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        c = np.asarray(cols, dtype=np.uint32)
        raise_for(_need("vcfc_query_samples_file")(self._h, in_path.encode(), query.reference_name,
                                                   len(query.reference_name), int(query.has_range), query.start,
                                                   query.end, c.ctypes.data, len(c), out_fd))

    def genotype_counts_buffer(self, data, query=None):
        """genotype-counts over .vcfc bytes, every record or
        (query: a VcfCoordinateQuery or a coordinate string) the matching
        ones.  Returns (status, record_indices, rows, samples): the counted
        records' file indices (uint64[n]), their rows n00 n01 n10 n11 n_other
        AN AC1 AC_other (uint32[n, 8]) and the per-sample table c00 c01 c10
        c11 c_other (uint64[S, 5]).  On VCFC_E_FORMAT the rows are those
        before the failing record (`last_counts_record`: its file index) and
        samples is None; any other failure returns no rows."""
        if query is not None and not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        src = np.frombuffer(data, dtype=np.uint8)
        ref = query.reference_name if query is not None else b""
        cap, scap = len(data) // 12 + 16, 4096
        while True:
            idx, rows = np.zeros(cap, dtype=np.uint64), np.zeros((cap, 8), dtype=np.uint32)
            tab = np.zeros((scap, 5), dtype=np.uint64)
            n, ns, bad = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            st = _need("vcfc_genotype_counts_buffer")(
                self._h, src.ctypes.data, len(data), int(query is not None), ref, len(ref),
                int(query.has_range) if query is not None else 0, query.start if query is not None else 0,
                query.end if query is not None else 0, idx.ctypes.data, rows.ctypes.data, cap, ctypes.byref(n),
                tab.ctypes.data, scap, ctypes.byref(ns), ctypes.byref(bad))
            if st == E_NOSPACE and (n.value > cap or ns.value > scap):
                cap, scap = max(cap, n.value), max(scap, ns.value)
                continue
            self.last_counts_record = bad.value
            return st, idx[:n.value].copy(), rows[:n.value].copy(), tab[:ns.value].copy() if st == OK else None

    def genotype_counts_file(self, in_path, variants_path, samples_path, query=None):
        """As `main genotype-counts <in.vcfc> <variants.tsv> <samples.tsv>
        [<query>]`: both TSV files (include/vcfc.h vcfc_genotype_counts_file)."""
        if query is not None and not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        ref = query.reference_name if query is not None else b""
        raise_for(_need("vcfc_genotype_counts_file")(
            self._h, in_path.encode(), variants_path.encode(), samples_path.encode(), int(query is not None), ref,
            len(ref), int(query.has_range) if query is not None else 0, query.start if query is not None else 0,
            query.end if query is not None else 0))

    def query_regions_buffer(self, data, regions, cap=None):
        """query-regions: the lines (no header) of the records
        matching at least one region, in file order, each once.  `regions` is
        region text (BED or <ref>[:<start>-<end>] lines) or a table from
        regions_build.  Returns (status, bytes): on VCFC_E_FORMAT the bytes
        are the matching records' lines before the record it stopped at."""
        tab = np.frombuffer(_regions_table(regions), dtype=np.uint8)
        src = np.frombuffer(data, dtype=np.uint8)
        cap = cap if cap is not None else 16 * len(data) + 4096
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint8)
            n = ctypes.c_uint64(0)
            st = _need("vcfc_query_regions_buffer")(self._h, src.ctypes.data, len(data), tab.ctypes.data, len(tab),
                                                    out.ctypes.data, cap, ctypes.byref(n))
            if st == E_NOSPACE and n.value > cap:
                cap = n.value
                continue
            return st, out[:n.value].tobytes()

    def query_regions_file(self, in_path, regions, out_fd=1):
        """As `main query-regions <file> <regions-file>`, with region text or a table."""
        tab = np.frombuffer(_regions_table(regions), dtype=np.uint8)
        raise_for(_need("vcfc_query_regions_file")(self._h, in_path.encode(), tab.ctypes.data, len(tab), out_fd))

    def query_samples_regions_buffer(self, data, regions, cols, cap=None):
        """query_samples_buffer over a region list.  Returns (status, bytes)."""
        tab = np.frombuffer(_regions_table(regions), dtype=np.uint8)
        src = np.frombuffer(data, dtype=np.uint8)
        c = np.asarray(cols, dtype=np.uint32)
        cap = cap if cap is not None else len(data) + 16 * len(c) * (len(data) // 64 + 1) + 4096
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint8)
            n = ctypes.c_uint64(0)
            st = _need("vcfc_query_samples_regions_buffer")(self._h, src.ctypes.data, len(data), tab.ctypes.data,
                                                            len(tab), c.ctypes.data, len(c), out.ctypes.data, cap,
                                                            ctypes.byref(n))
            if st == E_NOSPACE and n.value > cap:
                cap = n.value
                continue
            return st, out[:n.value].tobytes()

    def query_samples_regions_file(self, in_path, regions, cols, out_fd=1):
        tab = np.frombuffer(_regions_table(regions), dtype=np.uint8)
        c = np.asarray(cols, dtype=np.uint32)
        raise_for(_need("vcfc_query_samples_regions_file")(self._h, in_path.encode(), tab.ctypes.data, len(tab),
                                                           c.ctypes.data, len(c), out_fd))

    def genotype_counts_regions_buffer(self, data, regions):
        """genotype_counts_buffer over a region list: (status, record_indices,
        rows, samples), `last_counts_record` as there."""
        tab = np.frombuffer(_regions_table(regions), dtype=np.uint8)
        src = np.frombuffer(data, dtype=np.uint8)
        cap, scap = len(data) // 12 + 16, 4096
        while True:
            idx, rows = np.zeros(cap, dtype=np.uint64), np.zeros((cap, 8), dtype=np.uint32)
            st_tab = np.zeros((scap, 5), dtype=np.uint64)
            n, ns, bad = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            st = _need("vcfc_genotype_counts_regions_buffer")(
                self._h, src.ctypes.data, len(data), tab.ctypes.data, len(tab), idx.ctypes.data, rows.ctypes.data, cap,
                ctypes.byref(n), st_tab.ctypes.data, scap, ctypes.byref(ns), ctypes.byref(bad))
            if st == E_NOSPACE and (n.value > cap or ns.value > scap):
                cap, scap = max(cap, n.value), max(scap, ns.value)
                continue
            self.last_counts_record = bad.value
            return st, idx[:n.value].copy(), rows[:n.value].copy(), st_tab[:ns.value].copy() if st == OK else None

    def genotype_counts_regions_file(self, in_path, variants_path, samples_path, regions):
        """As `main genotype-counts-regions <in.vcfc> <variants.tsv> <samples.tsv> <regions-file>`."""
        tab = np.frombuffer(_regions_table(regions), dtype=np.uint8)
        raise_for(_need("vcfc_genotype_counts_regions_file")(self._h, in_path.encode(), variants_path.encode(),
                                                             samples_path.encode(), tab.ctypes.data, len(tab)))

    def genotype_matrix_buffer(self, data, layout, query=None, regions=None):
        """genotype-matrix over .vcfc bytes: one row per record,
        or per record matching `query` (a VcfCoordinateQuery or a coordinate
        string) or `regions` (region text or a table from regions_build).
        layout: GM_DOSAGE (int8[rows, S]), GM_HAP (int8[rows, 2 S]: h0, h1 per
        sample) or GM_BED (uint8[rows, ceil(S / 4)], PLINK 1 codes).  Returns
        (status, record_indices, matrix).  On VCFC_E_FORMAT the rows are those
        before the failing record (`last_matrix_record`: its file index); any
        other failure returns no rows."""
        if query is not None and regions is not None:
            raise ValueError("query and regions exclude each other")
        if query is not None and not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        src = np.frombuffer(data, dtype=np.uint8)
        tab = np.frombuffer(_regions_table(regions), dtype=np.uint8) if regions is not None else None
        ref = query.reference_name if query is not None else b""
        cap, nbytes = len(data) // 12 + 16, max(4 * len(data), 4096)
        while True:
            idx, rows = np.zeros(cap, dtype=np.uint64), np.zeros(nbytes, dtype=np.uint8)
            n, ns, bad = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            if tab is not None:
                st = _need("vcfc_genotype_matrix_regions_buffer")(
                    self._h, src.ctypes.data, len(data), layout, tab.ctypes.data, len(tab), idx.ctypes.data, cap,
                    rows.ctypes.data, nbytes, ctypes.byref(n), ctypes.byref(ns), ctypes.byref(bad))
            else:
                st = _need("vcfc_genotype_matrix_buffer")(
                    self._h, src.ctypes.data, len(data), layout, int(query is not None), ref, len(ref),
                    int(query.has_range) if query is not None else 0, query.start if query is not None else 0,
                    query.end if query is not None else 0, idx.ctypes.data, cap, rows.ctypes.data, nbytes, ctypes.byref(n),
                    ctypes.byref(ns), ctypes.byref(bad))
            rb = matrix_row_bytes(layout, ns.value)
            if st == E_NOSPACE and (n.value > cap or n.value * rb > nbytes):
                cap, nbytes = max(cap, n.value), max(nbytes, n.value * rb)
                continue
            self.last_matrix_record = bad.value
            m = rows[:n.value * rb].reshape(n.value, rb).copy()
            return st, idx[:n.value].copy(), m if layout == GM_BED else m.view(np.int8)

    def export_bed_file(self, in_path, prefix, query=None, regions=None):
        """As `main export-bed <in.vcfc> <prefix> [<query>]` or, with
        `regions`, `main export-bed-regions`: PLINK 1 <prefix>.bed / .bim / .fam."""
        if query is not None and regions is not None:
            raise ValueError("query and regions exclude each other")
        if regions is not None:
            tab = np.frombuffer(_regions_table(regions), dtype=np.uint8)
            raise_for(_need("vcfc_export_bed_regions_file")(self._h, in_path.encode(), prefix.encode(), tab.ctypes.data,
                                                            len(tab)))
            return
        if query is not None and not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        ref = query.reference_name if query is not None else b""
        raise_for(_need("vcfc_export_bed_file")(
            self._h, in_path.encode(), prefix.encode(), int(query is not None), ref, len(ref),
            int(query.has_range) if query is not None else 0, query.start if query is not None else 0,
            query.end if query is not None else 0))

    def ld_window_buffer(self, data, window, query=None, regions=None):
        """ld-window over .vcfc bytes: the 3 x 3 genotype tables
        of the pairs of rows (i, i + k), k = 1..window, the rows being
        genotype_matrix_buffer's (every record, or those matching `query` or
        `regions`).  Returns (status, record_indices, tables uint32[rows,
        window, 3, 3]): tables[i, k - 1, a, b] = the samples with genotype a in
        row i and b in row i + k, both called; zeros where row i + k does not
        exist.  On VCFC_E_FORMAT the band is that of the rows before the
        failing record (`last_ld_record`: its file index); any other failure
        returns no rows.  ld_r2(tables) gives r2."""
        if query is not None and regions is not None:
            raise ValueError("query and regions exclude each other")
        if query is not None and not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        src = np.frombuffer(data, dtype=np.uint8)
        tab = np.frombuffer(_regions_table(regions), dtype=np.uint8) if regions is not None else None
        ref = query.reference_name if query is not None else b""
        W = max(1, int(window)) if int(window) < 1 << 16 else 1
        cap = len(data) // 12 + 16
        while True:
            idx, tables = np.zeros(cap, dtype=np.uint64), np.zeros(cap * W * 9, dtype=np.uint32)
            n, bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
            if tab is not None:
                st = _need("vcfc_ld_window_regions_buffer")(
                    self._h, src.ctypes.data, len(data), window, tab.ctypes.data, len(tab), idx.ctypes.data, cap,
                    tables.ctypes.data, cap * W, ctypes.byref(n), ctypes.byref(bad))
            else:
                st = _need("vcfc_ld_window_buffer")(
                    self._h, src.ctypes.data, len(data), window, int(query is not None), ref, len(ref),
                    int(query.has_range) if query is not None else 0, query.start if query is not None else 0,
                    query.end if query is not None else 0, idx.ctypes.data, cap, tables.ctypes.data, cap * W,
                    ctypes.byref(n), ctypes.byref(bad))
            if st == E_NOSPACE and n.value > cap:
                cap = n.value
                continue
            self.last_ld_record = bad.value
            return st, idx[:n.value].copy(), tables[:n.value * W * 9].reshape(n.value, W, 3, 3).copy()

    def ld_window_file(self, in_path, out_tsv, window, min_r2=0.0, query=None, regions=None):
        """As `main ld-window <in.vcfc> <out.tsv> <window> <min-r2> [<query>]`
        or, with `regions`, `main ld-window-regions`: one text line per pair."""
        if query is not None and regions is not None:
            raise ValueError("query and regions exclude each other")
        if regions is not None:
            tab = np.frombuffer(_regions_table(regions), dtype=np.uint8)
            raise_for(_need("vcfc_ld_window_regions_file")(self._h, in_path.encode(), out_tsv.encode(), window, min_r2,
                                                           tab.ctypes.data, len(tab)))
            return
        if query is not None and not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        ref = query.reference_name if query is not None else b""
        raise_for(_need("vcfc_ld_window_file")(
            self._h, in_path.encode(), out_tsv.encode(), window, min_r2, int(query is not None), ref, len(ref),
            int(query.has_range) if query is not None else 0, query.start if query is not None else 0,
            query.end if query is not None else 0))

    def kinship_buffer(self, data, query=None, regions=None):
        """kinship over .vcfc bytes: the 3 x 3 genotype tables
        of every pair of samples over the rows of genotype_matrix_buffer
        (every record, or those matching `query` or `regions`).  Returns
        (status, record_indices, tables uint32[S, S, 3, 3]): tables[i, j, a, b]
        = the rows with genotype a in sample i and b in sample j, both called.
        On VCFC_E_FORMAT the square is that of the rows before the failing
        record (`last_kinship_record`: its file index); any other failure
        returns an empty square.  kinship_stats(tables) gives the statistics."""
        if query is not None and regions is not None:
            raise ValueError("query and regions exclude each other")
        if query is not None and not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        src = np.frombuffer(data, dtype=np.uint8)
        tab = np.frombuffer(_regions_table(regions), dtype=np.uint8) if regions is not None else None
        ref = query.reference_name if query is not None else b""
        # sized from the '#CHROM' line and the least record size; a short guess is reported and tried again
        raw = data if isinstance(data, (bytes, bytearray)) else src.tobytes()
        at = 0 if raw[:6] == b"#CHROM" else raw.find(b"\n#CHROM") + 1
        eol = raw.find(b"\n", at)
        S0 = max(0, raw[at:eol].count(b"\t") - 8) if eol > 0 else 0
        cap, tcap = len(data) // 12 + 16, S0 * S0
        while True:
            idx, tables = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(tcap, 1) * 9, dtype=np.uint32)
            n, S, bad = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            if tab is not None:
                st = _need("vcfc_kinship_regions_buffer")(
                    self._h, src.ctypes.data, len(data), tab.ctypes.data, len(tab), idx.ctypes.data, cap,
                    tables.ctypes.data, tcap, ctypes.byref(n), ctypes.byref(S), ctypes.byref(bad))
            else:
                st = _need("vcfc_kinship_buffer")(
                    self._h, src.ctypes.data, len(data), int(query is not None), ref, len(ref),
                    int(query.has_range) if query is not None else 0, query.start if query is not None else 0,
                    query.end if query is not None else 0, idx.ctypes.data, cap, tables.ctypes.data, tcap,
                    ctypes.byref(n), ctypes.byref(S), ctypes.byref(bad))
            if st == E_NOSPACE and (n.value > cap or S.value * S.value > tcap):
                cap, tcap = n.value, S.value * S.value
                continue
            self.last_kinship_record = bad.value
            if st not in (OK, E_FORMAT) or S.value * S.value > tcap:
                return st, idx[:0].copy(), np.zeros((0, 0, 3, 3), dtype=np.uint32)
            return st, idx[:n.value].copy(), tables[:S.value * S.value * 9].reshape(S.value, S.value, 3, 3).copy()

    def kinship_file(self, in_path, out_tsv, min_kinship=None, query=None, regions=None):
        """As `main kinship <in.vcfc> <out.tsv> <min-kinship|all> [<query>]` or,
        with `regions`, `main kinship-regions`: one text line per pair of
        samples (min_kinship None: every pair)."""
        if query is not None and regions is not None:
            raise ValueError("query and regions exclude each other")
        has_min, m = int(min_kinship is not None), float(min_kinship or 0.0)
        if regions is not None:
            tab = np.frombuffer(_regions_table(regions), dtype=np.uint8)
            raise_for(_need("vcfc_kinship_regions_file")(self._h, in_path.encode(), out_tsv.encode(), has_min, m,
                                                         tab.ctypes.data, len(tab)))
            return
        if query is not None and not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        ref = query.reference_name if query is not None else b""
        raise_for(_need("vcfc_kinship_file")(
            self._h, in_path.encode(), out_tsv.encode(), has_min, m, int(query is not None), ref, len(ref),
            int(query.has_range) if query is not None else 0, query.start if query is not None else 0,
            query.end if query is not None else 0))

    def extract_buffer(self, data, cols=None, query=None, regions=None, cap=None):
        """extract: the 0-based sample columns `cols` (None:
        all) of the records `query` or `regions` match (neither: all), as a
        .vcfc again.  Returns (status, bytes): on VCFC_E_FORMAT the bytes are
        the header and the records before the first one that is not regular
        or not re-encodable, a valid shorter .vcfc; VCFC_E_ARG (bad columns, a
        bad table) writes nothing."""
        if query is not None and regions is not None:
            raise ValueError("query and regions exclude each other")
        src = np.frombuffer(data, dtype=np.uint8)
        c = None if cols is None else np.asarray(cols, dtype=np.uint32)
        cp, k = (None, 0) if c is None else (c.ctypes.data, len(c))
        if c is not None and k == 0:
            cp = np.zeros(1, dtype=np.uint32).ctypes.data   # an empty list is not "all columns"
        tab = np.frombuffer(_regions_table(regions), dtype=np.uint8) if regions is not None else None
        if query is not None and not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        cap = cap if cap is not None else len(data) + 4096
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint8)
            n = ctypes.c_uint64(0)
            if tab is not None:
                st = _need("vcfc_extract_regions_buffer")(self._h, src.ctypes.data, len(data), cp, k, tab.ctypes.data,
                                                          len(tab), out.ctypes.data, cap, ctypes.byref(n))
            else:
                ref = query.reference_name if query is not None else b""
                st = _need("vcfc_extract_buffer")(
                    self._h, src.ctypes.data, len(data), cp, k, int(query is not None), ref, len(ref),
                    int(query.has_range) if query is not None else 0, query.start if query is not None else 0,
                    query.end if query is not None else 0, out.ctypes.data, cap, ctypes.byref(n))
            if st == E_NOSPACE and n.value > cap:
                cap = n.value
                continue
            return st, out[:n.value].tobytes()

    def extract_file(self, in_path, out_path, cols=None, query=None, regions=None):
        """As `main extract-samples <in> <out> <names> [<query>]` or, with
        `regions`, `main extract-regions <in> <out> <regions> [<names>]`, with
        columns in place of names."""
        if query is not None and regions is not None:
            raise ValueError("query and regions exclude each other")
        c = None if cols is None else np.asarray(cols, dtype=np.uint32)
        cp, k = (None, 0) if c is None else (c.ctypes.data, len(c))
        if c is not None and k == 0:
            cp = np.zeros(1, dtype=np.uint32).ctypes.data
        if regions is not None:
            tab = np.frombuffer(_regions_table(regions), dtype=np.uint8)
            raise_for(_need("vcfc_extract_regions_file")(self._h, in_path.encode(), out_path.encode(), cp, k,
                                                         tab.ctypes.data, len(tab)))
            return
        if query is not None and not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        ref = query.reference_name if query is not None else b""
        raise_for(_need("vcfc_extract_file")(
            self._h, in_path.encode(), out_path.encode(), cp, k, int(query is not None), ref, len(ref),
            int(query.has_range) if query is not None else 0, query.start if query is not None else 0,
            query.end if query is not None else 0))

    def sparse_query_status(self, in_path, query):
        """query_sparse_file_fd (reference src/main.cpp:235-582) over a sparse
        file: (status, stdout bytes); E_FORMAT where the reference throws (the
        bytes are every line it writes before)."""
        import tempfile
        if not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        with tempfile.TemporaryFile() as f:
            st = lib().vcfc_sparse_query_file(self._h, in_path.encode(), query.reference_name,
                                              len(query.reference_name), int(query.has_range), query.start,
                                              query.end, f.fileno())
            f.seek(0)
            return st, f.read()

    def sparse_query_file(self, in_path, query, out_fd=1):
        """Lines of a sparse file written to out_fd, as `main sparse-query`."""
        if not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        raise_for(lib().vcfc_sparse_query_file(self._h, in_path.encode(), query.reference_name,
                                               len(query.reference_name), int(query.has_range), query.start,
                                               query.end, out_fd))

    # -- binned external index (reference src/main.cpp:1284-1637, 2974-3349) --
    def create_binned_index_status(self, data, entries_per_bin):
        """create_binned_index4 over .vcfc bytes: (status, index bytes,
        err_record).  E_FORMAT where the reference throws (no bytes;
        err_record = the record), E_ARG for entries_per_bin == 0."""
        src = np.frombuffer(data, dtype=np.uint8)
        cap = 4096
        while True:
            out = np.empty(cap, dtype=np.uint8)
            n, er = ctypes.c_uint64(0), ctypes.c_int64(-1)
            st = _need("vcfc_create_binned_index_buffer")(self._h, src.ctypes.data, len(data), int(entries_per_bin),
                                                          out.ctypes.data, cap, ctypes.byref(n), ctypes.byref(er))
            if st == E_NOSPACE and n.value > cap:
                cap = n.value
                continue
            return st, out[:n.value].tobytes() if st == OK else b"", er.value

    def create_binned_index(self, data, entries_per_bin):
        """The bytes of <file>.vcfci for .vcfc bytes `data` (13-byte entries),
        raising where the reference throws."""
        st, out, er = self.create_binned_index_status(data, entries_per_bin)
        raise_for(st, "record %d" % er if er >= 0 else "")
        return out

    def create_binned_index_file(self, in_path, entries_per_bin, index_path=None):
        """`main create-binned-index <bin> <in_path>`: writes in_path + ".vcfci"
        (or index_path)."""
        index_path = index_path or in_path + ".vcfci"
        raise_for(_need("vcfc_create_binned_index_file")(self._h, in_path.encode(), index_path.encode(),
                                                         int(entries_per_bin)))

    def query_binned_index_status(self, data, index, query, cap=None):
        """query_binned_index_binarysearch over .vcfc bytes and their index
        bytes: (status, lines).  On E_FORMAT the bytes are every line written
        before the reference throws."""
        if not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        src = np.frombuffer(data, dtype=np.uint8)
        idx = np.frombuffer(index, dtype=np.uint8)
        cap = cap if cap is not None else 1 << 20
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint8)
            n = ctypes.c_uint64(0)
            st = _need("vcfc_query_binned_index_buffer")(self._h, src.ctypes.data, len(data),
                                                         idx.ctypes.data if len(index) else None, len(index),
                                                         query.reference_name, len(query.reference_name),
                                                         int(query.has_range), query.start, query.end,
                                                         out.ctypes.data, cap, ctypes.byref(n))
            if st == E_NOSPACE and n.value > cap:
                cap = n.value
                continue
            return st, out[:n.value].tobytes()

    def query_binned_index(self, data, index, query):
        """Like query_binned_index_status, raising where the reference throws."""
        st, out = self.query_binned_index_status(data, index, query)
        raise_for(st)
        return out

    def query_binned_index_file(self, in_path, query, out_fd=1, index_path=None):
        """`main query-binned-index <in_path> <region>`: lines to out_fd."""
        if not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        index_path = index_path or in_path + ".vcfci"
        raise_for(_need("vcfc_query_binned_index_file")(self._h, in_path.encode(), index_path.encode(),
                                                        query.reference_name, len(query.reference_name),
                                                        int(query.has_range), query.start, query.end, out_fd))

    # -- sparse external index (reference src/main.cpp:854-999, 1002-1281) and gap-analysis (:3931-3980) --
    def create_sparse_index_status(self, in_path, index_path=None):
        """create_sparse_external_index: writes in_path + ".vcfci-sparse" (or
        index_path), a sparse file with the 13-byte entry of a record at
        offset (300000000 + POS) * 256.  Returns (status, err_record,
        seek_failed): E_FORMAT where the reference throws (err_record = the
        record), seek_failed where its lseek to a slot fails (status OK);
        the entries of the records before it are in the file either way."""
        index_path = index_path or in_path + ".vcfci-sparse"
        er, sf = ctypes.c_int64(-1), ctypes.c_int(0)
        st = _need("vcfc_create_sparse_index_file")(self._h, in_path.encode(), index_path.encode(), ctypes.byref(er),
                                                    ctypes.byref(sf))
        return st, er.value, sf.value

    def create_sparse_index(self, in_path, index_path=None):
        """`main create-sparse-index <in_path>`, raising where the reference
        throws; returns True where its lseek failed and the index is partial."""
        st, er, sf = self.create_sparse_index_status(in_path, index_path)
        raise_for(st, "record %d" % er if er >= 0 else "")
        return bool(sf)

    def query_sparse_index(self, in_path, query, out_fd=1, index_path=None):
        """`main query-sparse-index <in_path> <region>`: lines to out_fd."""
        if not isinstance(query, VcfCoordinateQuery):
            query = parse_coordinate_string(query)
        index_path = index_path or in_path + ".vcfci-sparse"
        raise_for(_need("vcfc_query_sparse_index_file")(self._h, in_path.encode(), index_path.encode(),
                                                        query.reference_name, len(query.reference_name),
                                                        int(query.has_range), query.start, query.end, out_fd))

    @staticmethod
    def sparse_index_device(*args, **kw):
        """The module's sparse_index_device (no context state is used)."""
        return sparse_index_device(*args, **kw)

    def gap_analysis(self, in_path, out_path="start-positions.txt"):
        """`main gap-analysis <in_path>`: one line "<POS> <decoded line bytes>
        <compressed count>" per record into out_path."""
        raise_for(_need("vcfc_gap_analysis_file")(self._h, in_path.encode(), out_path.encode()))

    def sparsify_file(self, in_path, out_path):
        """sparsify_file (reference src/sparse.cpp:290-580)."""
        raise_for(lib().vcfc_sparsify_file(self._h, in_path.encode(), out_path.encode()))

    def sparsify_status(self, in_path, out_path):
        """sparsify_file without raising: the C status (VCFC_E_FORMAT where the
        reference throws, after writing the records before)."""
        return lib().vcfc_sparsify_file(self._h, in_path.encode(), out_path.encode())

    def sparsify_shard(self, in_path, out_path, rank, world):
        """This rank's slice of a sharded sparsify (vcfc_sparsify_shard):
        out_path None plans only.  Returns (status, [lo, hi, first_err or
        None, anomaly])."""
        info = (ctypes.c_uint64 * 4)()
        st = lib().vcfc_sparsify_shard(self._h, in_path.encode(), out_path.encode() if out_path else None,
                                       rank, world, info)
        return st, [info[0], info[1], None if info[2] == NO_ERROR else info[2], info[3]]

    def encode_rows(self, buf, line_off, line_len):
        """Host batch: returns (status, records bytes, rec_off, err_row)."""
        n = len(line_off)
        lo = np.ascontiguousarray(line_off, dtype=np.uint64)
        ll = np.ascontiguousarray(line_len, dtype=np.uint32)
        src = np.frombuffer(buf, dtype=np.uint8)
        cap = lib().vcfc_encode_bound(n, int(ll.sum(dtype=np.uint64))) + 16
        out = np.empty(cap, dtype=np.uint8)
        rec = np.zeros(n + 1, dtype=np.uint64)
        er = ctypes.c_int64(-1)
        st = lib().vcfc_encode_rows(self._h, src.ctypes.data, len(buf), lo.ctypes.data, ll.ctypes.data, n,
                                    out.ctypes.data, cap, rec.ctypes.data, ctypes.byref(er))
        upto = n if st == OK else max(er.value, 0)
        return st, out[:int(rec[upto])].tobytes(), rec, er.value


# -- device-pointer API (used with torch tensors in bench.py / GPU tests) ----
def workspace_size(n_rows, total_line_bytes):
    return int(lib().vcfc_encode_workspace_size(n_rows, total_line_bytes))


def encode_bound(n_rows, total_line_bytes):
    return int(lib().vcfc_encode_bound(n_rows, total_line_bytes))


def encode_rows_device(d_buf, d_line_off, d_line_len, n, total_line_bytes, d_out, out_cap, d_rec_off,
                       d_ws, ws_bytes, d_err, stream=0):
    st = lib().vcfc_encode_rows_device(d_buf, d_line_off, d_line_len, n, total_line_bytes, d_out, out_cap,
                                       d_rec_off, d_ws, ws_bytes, d_err, stream)
    raise_for(st)


def _need(name):
    """The export `name` of the loaded library (an older build loaded through
    VCFC_LIB may lack it: a clear error instead of an AttributeError)."""
    L = lib()
    if not hasattr(L, name):
        raise RuntimeError("%s: %s is not exported by this build of libvcfc.so" % (LIB_PATH, name))
    return getattr(L, name)


def encode_deferred_rows(d_ws, n, total_line_bytes, stream=0):
    """Rows the last encode_rows_device on workspace d_ws deferred (waits for stream)."""
    v = ctypes.c_uint64(0)
    raise_for(_need("vcfc_encode_deferred_rows")(d_ws, n, total_line_bytes, stream, ctypes.byref(v)))
    return int(v.value)


class StageTimer:
    """Per-stage HIP-event timing of encode_rows_device (see vcfc_timer_read)."""
    STAGES = ("slot_scan", "k_encode", "size_scan", "k_compact")

    def __init__(self):
        self._h = ctypes.c_void_p()
        raise_for(lib().vcfc_timer_create(ctypes.byref(self._h)))

    def encode(self, d_buf, d_line_off, d_line_len, n, total_line_bytes, d_out, out_cap, d_rec_off,
               d_ws, ws_bytes, d_err, stream=0):
        raise_for(lib().vcfc_encode_rows_device_timed(d_buf, d_line_off, d_line_len, n, total_line_bytes, d_out,
                                                      out_cap, d_rec_off, d_ws, ws_bytes, d_err, stream, self._h))

    def read(self):
        ms = (ctypes.c_double * 4)()
        calls = ctypes.c_uint64(0)
        raise_for(lib().vcfc_timer_read(self._h, ms, ctypes.byref(calls)))
        return dict(zip(self.STAGES, list(ms))), calls.value

    def __del__(self):
        try:
            lib().vcfc_timer_destroy(self._h)
        except Exception:
            pass


def decode_workspace_size(n_records):
    return int(lib().vcfc_decode_workspace_size(n_records))


def decode_records_device(d_in, in_bytes, d_rec_start, n, samples, d_out, out_cap, d_line_off, d_ws, ws_bytes,
                          d_err, stream=0, exact=False):
    raise_for(lib().vcfc_decode_records_device(d_in, in_bytes, d_rec_start, n, samples, d_out, out_cap, d_line_off,
                                               d_ws, ws_bytes, d_err, int(exact), stream))


def decode_selected_device(d_in, in_bytes, d_rec_start, d_select, n, samples, d_out, out_cap, d_line_off, d_ws,
                           ws_bytes, d_err, stream=0, exact=False):
    raise_for(lib().vcfc_decode_selected_device(d_in, in_bytes, d_rec_start, d_select, n, samples, d_out, out_cap,
                                                d_line_off, d_ws, ws_bytes, d_err, int(exact), stream))


def query_match_device(d_in, d_rec_start, n, d_ref, ref_len, has_range, start, end, d_flag, d_err, stream=0):
    """Device match step of the range query (see include/vcfc.h)."""
    return lib().vcfc_query_match_device(d_in, d_rec_start, n, d_ref, ref_len, int(has_range), start, end, d_flag,
                                         d_err, stream)


REGIONS_MAGIC = b"VCRG"   # the first bytes of a region table (csrc/vcfc_device.h VCFC_REGIONS_MAGIC)


def regions_build(text):
    """The region table (bytes) of region text, one region per line: BED
    (name TAB start TAB end, 0-based half-open) or <ref>[:<start>-<end>]
    (include/vcfc.h vcfc_regions_build).  Raises ValueError naming the
    1-based line that does not parse."""
    text = text.encode() if isinstance(text, str) else bytes(text)
    nb, nr, bad = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    f = _need("vcfc_regions_build")
    st = f(text, len(text), None, 0, ctypes.byref(nb), ctypes.byref(nr), ctypes.byref(bad))
    out = np.zeros(max(nb.value, 1), dtype=np.uint8)
    if st == E_NOSPACE:
        st = f(text, len(text), out.ctypes.data, nb.value, ctypes.byref(nb), ctypes.byref(nr), ctypes.byref(bad))
    if st == E_ARG and bad.value:
        line = text.split(b"\n")[bad.value - 1].rstrip(b"\r")
        raise ValueError("Failed to parse region at line %d: %s" % (bad.value, line.decode(errors="replace")))
    raise_for(st)
    return out[:nb.value].tobytes()


def _regions_table(regions):
    """A table as it is; region text built."""
    if isinstance(regions, (bytes, bytearray)) and bytes(regions[:4]) == REGIONS_MAGIC:
        return bytes(regions)
    return regions_build(regions)


def regions_workspace_size(table_bytes):
    return int(_need("vcfc_regions_workspace_size")(table_bytes))


def regions_upload(table, d_ws, ws_bytes, stream=0):
    """Validate a table from regions_build and copy it into the device
    workspace d_ws (include/vcfc.h vcfc_regions_upload).  Returns the status."""
    t = np.frombuffer(table, dtype=np.uint8)
    return _need("vcfc_regions_upload")(t.ctypes.data if len(t) else None, len(t), d_ws, ws_bytes, stream)


def regions_match_device(d_in, d_rec_start, n, d_ws, ws_bytes, d_flag, d_err, stream=0):
    """query_match_device with the table uploaded into d_ws in place of one
    region.  Returns the status; enqueued on `stream`."""
    return _need("vcfc_regions_match_device")(d_in, d_rec_start, n, d_ws, ws_bytes, d_flag, d_err, stream)


def synth_rows_device(d_buf, d_line_off, n, d_prefix, d_prefix_off, d_row_af, samples, law, seed, stream=0,
                      row_base=0):
    st = lib().vcfc_synth_rows_device_at(d_buf, d_line_off, n, d_prefix, d_prefix_off, d_row_af, samples,
                                         law, seed, row_base, stream)
    raise_for(st)


def record_hash_device(d_recs, d_rec_off, n, d_hash, stream=0):
    """Per-record 64-bit digests on the GPU (include/vcfc.h vcfc_record_hash_device)."""
    raise_for(lib().vcfc_record_hash_device(d_recs, d_rec_off, n, d_hash, stream))


def sparse_plan_device(d_recs, d_rec_off, n, data_start, d_file_off, d_prefix16, d_status, stream=0):
    """The sparse layout of device-resident records (include/vcfc.h
    vcfc_sparse_plan_device): file offsets, 16-byte prefixes and the two
    status words, enqueued on `stream`."""
    raise_for(lib().vcfc_sparse_plan_device(d_recs, d_rec_off, n, data_start, d_file_off, d_prefix16, d_status,
                                            stream))


def sparse_index_workspace_size(n_records):
    return int(_need("vcfc_sparse_index_workspace_size")(n_records))


def sparse_index_offset(pos):
    """The file offset of the slot of `pos` in a sparse external index."""
    return int(_need("vcfc_sparse_index_offset")(pos))


def sparse_index_device(d_in, d_rec_start, n, base_offset, d_entries, d_file_off, d_count, d_status, d_ws, ws_bytes,
                        d_err, stream=0):
    """The kept entries of device-resident records and their file offsets
    (include/vcfc.h vcfc_sparse_index_device); enqueued on `stream`."""
    raise_for(_need("vcfc_sparse_index_device")(d_in, d_rec_start, n, base_offset, d_entries, d_file_off, d_count,
                                                d_status, d_ws, ws_bytes, d_err, stream))


def decode_sizes_workspace_size(n_records):
    return int(_need("vcfc_decode_sizes_workspace_size")(n_records))


def decode_sizes_device(d_in, in_bytes, d_rec_start, n, sample_count, d_line_off, d_pos_off, d_pos_len, d_ccount,
                        d_ws, ws_bytes, d_err, stream=0):
    """Decoded line offsets without the lines, and per record the POS text
    location and the reference's compressed count (include/vcfc.h
    vcfc_decode_sizes_device); enqueued on `stream`."""
    raise_for(_need("vcfc_decode_sizes_device")(d_in, in_bytes, d_rec_start, n, sample_count, d_line_off, d_pos_off,
                                                d_pos_len, d_ccount, d_ws, ws_bytes, d_err, stream))


def index_workspace_size(n_records):
    return int(_need("vcfc_index_workspace_size")(n_records))


def binned_index_device(d_in, d_rec_start, n, base_offset, entries_per_bin, d_entries, entries_cap, d_count, d_info,
                        d_ws, ws_bytes, d_err, stream=0):
    """The packed index entries of device-resident records (include/vcfc.h
    vcfc_binned_index_device); enqueued on `stream`."""
    raise_for(_need("vcfc_binned_index_device")(d_in, d_rec_start, n, base_offset, entries_per_bin, d_entries,
                                                entries_cap, d_count, d_info, d_ws, ws_bytes, d_err, stream))


def record_span_device(d_in, d_rec_start, n, d_ref_idx, d_pos, d_end, d_err, stream=0):
    """Per record ref_idx (u8), POS and end position (u64 each) on the GPU."""
    raise_for(_need("vcfc_record_span_device")(d_in, d_rec_start, n, d_ref_idx, d_pos, d_end, d_err, stream))


def sample_columns(data, names):
    """The 0-based sample columns of `names` (a list of names, or one
    comma-separated string) in the '#CHROM' line of .vcfc bytes (the header
    is enough), in list order.  Raises ValueError for a name the header does
    not hold or a name listed twice."""
    nb = names if isinstance(names, (bytes, str)) else b",".join(x.encode() if isinstance(x, str) else x for x in names)
    nb = nb.encode() if isinstance(nb, str) else bytes(nb)
    src = np.frombuffer(data, dtype=np.uint8)
    cap = nb.count(b",") + 1
    cols = np.zeros(cap, dtype=np.uint32)
    n, bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    st = _need("vcfc_sample_columns")(src.ctypes.data, len(data), nb, len(nb), cols.ctypes.data, cap, ctypes.byref(n),
                                      ctypes.byref(bad))
    if st == E_ARG:
        name = nb[bad.value:].split(b",")[0]
        kind = "Duplicate" if name in nb[:bad.value].split(b",")[:-1] else "Unknown"
        raise ValueError("%s sample name: %s" % (kind, name.decode(errors="replace")))
    raise_for(st)
    return [int(x) for x in cols[:n.value]]


def subset_workspace_size(n_records, n_cols):
    return int(_need("vcfc_subset_workspace_size")(n_records, n_cols))


def decode_samples_device(d_in, in_bytes, d_rec_start, d_select, n, samples, cols, d_out, out_cap, d_line_off, d_ws,
                          ws_bytes, d_err, stream=0):
    """The lines of device-resident records cut to the sample columns `cols`
    (host list; include/vcfc.h vcfc_decode_samples_device); d_select may be
    None.  Returns the status (VCFC_E_ARG for bad columns); enqueued on
    `stream`."""
    c = np.asarray(cols, dtype=np.uint32)
    return _need("vcfc_decode_samples_device")(d_in, in_bytes, d_rec_start, d_select, n, samples, c.ctypes.data, len(c),
                                               d_out, out_cap, d_line_off, d_ws, ws_bytes, d_err, stream)


def extract_bound(in_bytes, n_records, n_cols):
    return int(_need("vcfc_extract_bound")(in_bytes, n_records, n_cols))


def extract_workspace_size(n_records, n_cols):
    """n_cols: the chosen columns (all columns: the sample count)."""
    return int(_need("vcfc_extract_workspace_size")(n_records, n_cols))


def extract_samples_device(d_in, in_bytes, d_rec_start, d_select, n, samples, cols, d_out, out_cap, d_rec_off, d_ws,
                           ws_bytes, d_err, stream=0):
    """Device-resident records cut to the sample columns `cols` (host list;
    None: all) and written as .vcfc records at d_out + d_rec_off[i]
    (include/vcfc.h vcfc_extract_samples_device); d_select may be None.
    Returns the status (VCFC_E_ARG for bad columns); enqueued on `stream`."""
    c = None if cols is None else np.asarray(cols, dtype=np.uint32)
    cp, k = (None, 0) if c is None else (c.ctypes.data, len(c))
    if c is not None and k == 0:
        cp = np.zeros(1, dtype=np.uint32).ctypes.data
    return _need("vcfc_extract_samples_device")(d_in, in_bytes, d_rec_start, d_select, n, samples, cp, k, d_out, out_cap,
                                                d_rec_off, d_ws, ws_bytes, d_err, stream)


def counts_workspace_size(n_records, samples):
    return int(_need("vcfc_counts_workspace_size")(n_records, samples))


def counts_lds_samples():
    """The largest sample count whose histogram the counts kernel sums in LDS."""
    return int(_need("vcfc_counts_lds_samples")())


def counts_trip_records(samples, with_sample_table=True):
    """The records one pass of the counts kernel's resident grid covers on the
    current device, with or without the sample table."""
    return int(_need("vcfc_counts_trip_records")(samples, int(bool(with_sample_table))))


def genotype_counts_device(d_in, in_bytes, d_rec_start, d_select, n, samples, d_variant, d_sample, d_ws, ws_bytes, d_err,
                           stream=0):
    """Rows (d_variant: 8 n uint32) and the per-sample table (d_sample: 5 S
    uint64, added to) of device-resident records (include/vcfc.h
    vcfc_genotype_counts_device); d_select, d_variant, d_sample may be None.
    Returns the status; enqueued on `stream`."""
    return _need("vcfc_genotype_counts_device")(d_in, in_bytes, d_rec_start, d_select, n, samples, d_variant, d_sample,
                                                d_ws, ws_bytes, d_err, stream)


GM_DOSAGE, GM_HAP, GM_BED = 0, 1, 2   # include/vcfc.h VCFC_GM_*


def matrix_row_bytes(layout, samples):
    """Bytes of a genotype-matrix row (0 for an unknown layout)."""
    return int(_need("vcfc_matrix_row_bytes")(layout, samples))


def matrix_lds_samples(layout):
    """The largest sample count whose row the matrix kernel puts together in LDS."""
    return int(_need("vcfc_matrix_lds_samples")(layout))


def matrix_trip_records(layout):
    """The records one pass of the matrix kernel's resident grid covers on the current device."""
    return int(_need("vcfc_matrix_trip_records")(layout))


def matrix_workspace_size(n_records, samples, layout):
    return int(_need("vcfc_matrix_workspace_size")(n_records, samples, layout))


def genotype_matrix_device(d_in, in_bytes, d_rec_start, d_select, n, samples, layout, d_out, out_cap, row_stride,
                           d_row_of, d_ws, ws_bytes, d_err, stream=0):
    """The genotype-matrix rows of device-resident records (include/vcfc.h
    vcfc_genotype_matrix_device): record i's row at d_out + d_row_of[i] *
    row_stride; d_select may be None.  Pointers or torch tensors' data_ptr().
    Returns the status; enqueued on `stream`."""
    return _need("vcfc_genotype_matrix_device")(d_in, in_bytes, d_rec_start, d_select, n, samples, layout, d_out, out_cap,
                                                row_stride, d_row_of, d_ws, ws_bytes, d_err, stream)


def ld_workspace_size(n_records, samples, window):
    return int(_need("vcfc_ld_workspace_size")(n_records, samples, window))


def ld_tables_device(d_bed, n_rows, row_stride, samples, window, d_tables, pairs_cap, d_ws, ws_bytes, d_err, stream=0):
    """The genotype tables of device-resident .bed rows (include/vcfc.h
    vcfc_ld_tables_device): slot i * window + k - 1 of d_tables (nine uint32)
    is the table of rows (i, i + k).  Asynchronous on `stream`."""
    return _need("vcfc_ld_tables_device")(d_bed, n_rows, row_stride, samples, window, d_tables, pairs_cap, d_ws, ws_bytes,
                                          d_err, stream)


def ld_window_device(d_in, in_bytes, d_rec_start, d_select, n, samples, window, d_tables, pairs_cap, d_row_of, d_ws,
                     ws_bytes, d_err, stream=0):
    """The composed call on device-resident records (include/vcfc.h
    vcfc_ld_window_device): .bed rows into the workspace, bit planes, pairs;
    d_row_of[n] = the rows.  Asynchronous on `stream`, capturable."""
    return _need("vcfc_ld_window_device")(d_in, in_bytes, d_rec_start, d_select, n, samples, window, d_tables, pairs_cap,
                                          d_row_of, d_ws, ws_bytes, d_err, stream)


def ld_r2(tables):
    """r2 of genotype tables (any shape ending in 3, 3, or in 9): float64, nan
    where it is undefined (no variance in either row among the samples called
    in both).  Integers exact in int64, then ((double)cov * (double)cov) /
    ((double)vx * (double)vy), as the C library's text output."""
    t = np.asarray(tables).astype(np.int64)
    t = t.reshape(t.shape[:-1] + (3, 3)) if t.shape[-1] == 9 else t
    a = np.arange(3, dtype=np.int64)
    row, col = t.sum(axis=-1), t.sum(axis=-2)
    N = row.sum(axis=-1)
    sx, sy = (row * a).sum(axis=-1), (col * a).sum(axis=-1)
    sxx, syy = (row * a * a).sum(axis=-1), (col * a * a).sum(axis=-1)
    sxy = (t * np.outer(a, a)).sum(axis=(-1, -2))
    cov, vx, vy = N * sxy - sx * sy, N * sxx - sx * sx, N * syy - sy * sy
    ok = (vx != 0) & (vy != 0)
    c = cov.astype(np.float64)
    den = np.where(ok, vx.astype(np.float64) * vy.astype(np.float64), 1.0)
    return np.where(ok, (c * c) / den, np.nan)


def kin_workspace_size(n_records, samples):
    return int(_need("vcfc_kin_workspace_size")(n_records, samples))


def kin_tables_device(d_bed, n_rows, row_stride, samples, d_tables, tables_cap, accumulate, d_ws, ws_bytes, d_err, stream=0):
    """The genotype tables of every pair of samples over device-resident .bed
    rows (include/vcfc.h vcfc_kin_tables_device): table (i, j) at d_tables +
    (i * samples + j) * 9 uint32; accumulate != 0 adds to what d_tables holds.
    Asynchronous on `stream`."""
    return _need("vcfc_kin_tables_device")(d_bed, n_rows, row_stride, samples, d_tables, tables_cap, accumulate, d_ws,
                                           ws_bytes, d_err, stream)


def kin_records_device(d_in, in_bytes, d_rec_start, d_select, n, samples, d_tables, tables_cap, accumulate, d_row_of, d_ws,
                       ws_bytes, d_err, stream=0):
    """The composed call on device-resident records (include/vcfc.h
    vcfc_kin_records_device): .bed rows into the workspace, sample-major bit
    planes, pairs; d_row_of[n] = the rows.  Asynchronous on `stream`,
    capturable."""
    return _need("vcfc_kin_records_device")(d_in, in_bytes, d_rec_start, d_select, n, samples, d_tables, tables_cap,
                                            accumulate, d_row_of, d_ws, ws_bytes, d_err, stream)


def kinship_stats(tables):
    """(N, IBS0, IBS1, IBS2, DST, KINSHIP) of genotype tables (any shape ending
    in 3, 3, or in 9): int64 arrays, and float64 with nan where
    undefined (DST: N == 0; KINSHIP, the KING-robust between-family estimator:
    min(HET_A, HET_B) == 0).  Integers exact in int64, then one conversion per
    operand and one division, as the C library's text output."""
    t = np.asarray(tables).astype(np.int64)
    t = t.reshape(t.shape[:-2] + (9,)) if t.shape[-1] == 3 else t
    N = t.sum(axis=-1)
    ibs0 = t[..., 2] + t[..., 6]
    ibs2 = t[..., 0] + t[..., 4] + t[..., 8]
    ibs1 = N - ibs0 - ibs2
    hh = t[..., 4]
    het_a, het_b = t[..., 3] + hh + t[..., 5], t[..., 1] + hh + t[..., 7]
    m = np.minimum(het_a, het_b)
    dst = np.where(N != 0, (2 * ibs2 + ibs1).astype(np.float64) / np.where(N != 0, 2 * N, 1).astype(np.float64), np.nan)
    num = 2 * hh - 4 * ibs0 + 2 * m - het_a - het_b
    kin = np.where(m != 0, num.astype(np.float64) / np.where(m != 0, 4 * m, 1).astype(np.float64), np.nan)
    return N, ibs0, ibs1, ibs2, dst, kin
