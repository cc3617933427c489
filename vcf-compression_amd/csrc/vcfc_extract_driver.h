// vcfc_extract_driver.h -- host side of extract, shared by
// the C ABI (vcfc_api.cpp) and the CPU emulator harness
// (tests/simt_emu/emu_extract_api.cpp), so the same control flow is tested on
// both.
//
// The driver is the sample-subset decoder's (vcfc_subset_driver.h) run with
// extract's kernels:
//   1. the header, always: '##' lines verbatim, the '#CHROM' line cut as the
//      sample-subset decoder cuts it (verbatim with no column list:
//      vcfc_ext::Call);
//   2. extract_section = vcfc_sub::subset_section(EXTRACT, ...): the plan is exact
//      over record sizes and stops at the first taken record that is not
//      regular or not re-encodable; the records before it are written
//      densely.
#pragma once
#include <cstdint>

#include "vcfc_subset_driver.h"

namespace vcfc_ext {

using vcfc_sub::ST_E_ARG;
using vcfc_sub::ST_E_FORMAT;
using vcfc_sub::ST_E_HIP;
using vcfc_sub::ST_E_IO;
using vcfc_sub::ST_OK;

constexpr vcfc_sub::Kernels EXTRACT = {vcfc_extract_workspace_layout, vcfc_extract_plan, vcfc_extract_write};

// An upper bound on the bytes of an extract of n_records records, K columns,
// out of a file of in_bytes: the header is never longer than the input's; a
// record keeps its headers, REQ and LF, a chosen class token costs at most
// one run byte, and another chosen token its source bytes and terminator plus
// its own 0xE1 -- at most one byte a chosen column, and one for the source's
// last token, which has no terminator of its own.
inline uint64_t extract_bound(uint64_t in_bytes, uint64_t n_records, uint64_t K) { return in_bytes + n_records * (K + 1); }

// Header and sorted columns of an extract call: vcfc_sub::Call with its
// option on (cols == nullptr and K == 0: every column, in file order).
struct Call : vcfc_sub::Call {
    int prepare(const uint8_t *in, uint64_t n, const uint32_t *cols, uint64_t K) {
        return vcfc_sub::Call::prepare(in, n, cols, K, true);
    }
};

// The device entry's columns: the list, or 0 .. S - 1.
inline int device_columns(const uint32_t *cols, uint64_t K, uint64_t S, std::vector<uint32_t> &csort,
                          std::vector<uint32_t> &rank) {
    return vcfc_sub::choose_columns(cols, K, S, true, csort, rank);
}

// The records (no header) of a .vcfc data section: all of them (match ==
// nullptr), or those `match` flags.  vcfc_sub::subset_section with extract's
// kernels.
inline int extract_section(const uint8_t *h_in, uint64_t n, uint64_t S, const std::vector<uint32_t> &csort,
                           const std::vector<uint32_t> &rank, const vcfc_dec::MatchStep *match, vcfc_dec::Buffers &B,
                           hipStream_t s, const vcfc_dec::Sink &sink, uint64_t out_batch = 1ull << 30) {
    return vcfc_sub::subset_section(EXTRACT, h_in, n, S, csort, rank, match, B, s, sink, out_batch);
}

}  // namespace vcfc_ext
