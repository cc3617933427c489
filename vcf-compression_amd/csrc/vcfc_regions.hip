// vcfc_regions.hip -- gfx950 kernel for region-list queries.
//
// k_regions_match is k_query_match with a table in place of one region: one
// lane per record through query_frame (vcfc_query_dev.h: the two 16-byte
// loads, the SWAR TAB search, the LDS copy, pos_parse, the byte-serial path,
// the error word), then per lane
//   1. a binary search of the record's CHROM among the table's names, sorted
//      by (length, bytes): the byte compares read the lane's LDS copy;
//   2. a binary search of that name's interval starts for the last one
//      <= POS; the record matches iff POS <= that interval's end;
//   3. the same interval search under the wildcard name, if the table has it.
// The table is read through global memory: the records of a wave share their
// CHROM and have nearby POS, so their probes fall on the same cache lines.
// The kernel trusts the table: vcfc_regions_upload validated it on the host.
#include <hip/hip_runtime.h>
#include "vcfc_device.h"
#include "vcfc_query_dev.h"

namespace {

struct RegTable {
    const VcfcRegionName *names;
    const uint8_t *bytes;
    const uint64_t *starts, *ends;
    uint32_t n_names;
};

// POS inside one of the name's disjoint, sorted intervals
__device__ __forceinline__ bool regions_hit(const RegTable &T, const VcfcRegionName &nm, uint64_t pos) {
    const uint64_t *st = T.starts + nm.iv_first;
    uint32_t lo = 0, hi = nm.iv_count;   // first start > pos
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (st[mid] <= pos) lo = mid + 1;
        else hi = mid;
    }
    return lo != 0 && pos <= T.ends[nm.iv_first + lo - 1];
}

// <0, 0, >0: (len, name) against table name k in (length, bytes) order
__device__ __forceinline__ int regions_cmp(const RegTable &T, const VcfcRegionName &nm, const uint8_t *name, uint64_t len) {
    if (len != nm.len) return len < nm.len ? -1 : 1;
    const uint8_t *b = T.bytes + nm.byte_off;
    for (uint32_t k = 0; k < nm.len; k++)
        if (name[k] != b[k]) return name[k] < b[k] ? -1 : 1;
    return 0;
}

__device__ __forceinline__ bool regions_matches(const RegTable &T, const uint8_t *name, uint64_t len, uint64_t pos) {
    if (T.n_names == 0) return false;
    bool m = false;
    const VcfcRegionName first = T.names[0];
    const bool wild = first.len == 0;
    if (wild) m = regions_hit(T, first, pos);
    if (m || len == 0) return m;   // an empty CHROM has only the wildcard's intervals
    uint32_t lo = wild ? 1u : 0u, hi = T.n_names;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const VcfcRegionName nm = T.names[mid];
        const int c = regions_cmp(T, nm, name, len);
        if (c == 0) return regions_hit(T, nm, pos);
        if (c < 0) hi = mid;
        else lo = mid + 1;
    }
    return false;
}

__global__ __launch_bounds__(256) void k_regions_match(const uint8_t *in, const uint64_t *rec, uint64_t n,
                                                       const uint8_t *table, uint8_t *flag, uint64_t *err) {
    __shared__ __attribute__((aligned(16))) uint8_t win[256 * QM_WIN];
    const VcfcRegionsHeader *h = reinterpret_cast<const VcfcRegionsHeader *>(table);
    RegTable T;
    T.names = reinterpret_cast<const VcfcRegionName *>(table + h->off_names);
    T.bytes = table + h->off_bytes;
    T.starts = reinterpret_cast<const uint64_t *>(table + h->off_starts);
    T.ends = reinterpret_cast<const uint64_t *>(table + h->off_ends);
    T.n_names = h->n_names;
    query_frame(in, rec, n, win, flag, err,
                [&](const uint8_t *name, uint64_t name_len, uint64_t pos) { return regions_matches(T, name, name_len, pos); });
}

// the error word in a launch of its own, so the call can be captured
__global__ void k_regions_reset(uint64_t *err) {
    if (threadIdx.x == 0) *err = ~0ull;
}

}  // namespace

hipError_t vcfc_regions_match(const uint8_t *in, const uint64_t *rec_start, uint64_t n, const uint8_t *table,
                              uint8_t *flag, uint64_t *err, hipStream_t s) {
    hipLaunchKernelGGL(k_regions_reset, dim3(1), dim3(64), 0, s, err);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(k_regions_match, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, rec_start, n, table, flag,
                       err);
    return hipGetLastError();
}
