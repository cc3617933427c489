// vcfc_index.hip -- gfx950 kernels of the binned external index
// (create-binned-index / query-binned-index; reference create_binned_index4,
// src/main.cpp:1284-1637, compute_end_position :763-852,
// query_binned_index_binarysearch :2974-3349, compare_to_range :110-137).
//
//   k_index_span     one lane per record: ref_idx, POS and the end position
//   k_idx_blockmax   per-block maximum of end                     } inclusive
//   k_idx_partials   exclusive prefix maximum of the block maxima } 64-bit
//   k_idx_flags      prefix maximum M_i and the open flags        } prefix max
//   (vcfc_scan_u32   entry number of every record)
//   k_idx_emit       the packed 13-byte entries, their count, the largest end
//   k_index_compare  a query against ref_idx / pos / end: select flags and
//                    the first record after the query
//
// Every cross-lane step uses csrc/vcfc_wave.h only, so tests/simt_emu runs
// this file on the CPU.
#include <hip/hip_runtime.h>
#include <vcfc_wave.h>   // angle brackets: tests/simt_emu shadows it
#include "vcfc_device.h"

namespace {

constexpr uint32_t IDX_THREADS = 256;

#include "vcfc_index_dev.h"   // field parsers and the SWAR TAB search (shared with vcfc_sparse_index.hip)

// Byte-serial span of the record in[rs, re): 0, or code 2 / 3.
__device__ uint32_t idx_span_seq(const uint8_t *in, uint64_t rs, uint64_t re, uint32_t *ref, uint64_t *pos,
                                 uint64_t *end) {
    uint64_t t[8];
    uint64_t k = rs + 8;
    for (uint32_t f = 0; f < 8; f++) {
        while (k < re && in[k] != '\t') k++;
        if (k >= re) return 3;
        t[f] = k++;
    }
    const uint8_t *chrom = in + rs + 8;
    *ref = idx_ref(chrom, t[0] - (rs + 8));
    if (!idx_strtoul(in + t[0] + 1, t[1] - t[0] - 1, pos)) return 2;
    bool sv = false;
    const uint64_t alt = idx_alt_longest(in + t[3] + 1, t[4] - t[3] - 1, &sv);
    if (sv) return idx_sv_end(in + t[6] + 1, t[7] - t[6] - 1, *pos, end) ? 0u : 2u;
    const uint64_t rl = t[3] - t[2] - 1;
    *end = *pos + (rl >= alt ? rl : alt) - 1;
    return 0;
}

// One lane per record.  Fast path: the 48 bytes from the CHROM start lie
// inside the record and hold the first five TABs (CHROM .. ALT), and ALT is
// not structural: three 16-byte loads, TABs found by SWAR in registers, the
// fields parsed from an LDS copy; the three TABs after ALT are then only
// counted (16-byte loads below the record end).  Otherwise byte by byte.
constexpr uint32_t IS_WIN = 48;
__global__ __launch_bounds__(256) void k_index_span(const uint8_t *in, const uint64_t *rec, uint64_t n,
                                                    uint8_t *ref_idx, uint64_t *pos_out, uint64_t *end_out,
                                                    uint64_t *err) {
    __shared__ __attribute__((aligned(16))) uint8_t win[IDX_THREADS * IS_WIN];
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t rs = rec[i], re = rec[i + 1];
    uint32_t ref = 0, code = 0;
    uint64_t pos = 0, end = 0;
    bool done = false;
    if (re >= rs + 8 + IS_WIN) {
        const uint8_t *p = in + rs + 8;
        const uint4 v0 = vw::uload16(p), v1 = vw::uload16(p + 16), v2 = vw::uload16(p + 32);
        uint8_t *f = win + threadIdx.x * IS_WIN;
        uint4 *w = reinterpret_cast<uint4 *>(f);
        w[0] = v0; w[1] = v1; w[2] = v2;
        uint64_t m = tab_bits16(v0) | tab_bits16(v1) << 16 | tab_bits16(v2) << 32;
        uint32_t t[5];
        bool five = true;
        for (uint32_t k = 0; k < 5; k++) {
            five = five && m != 0;
            t[k] = m ? (uint32_t)__builtin_ctzll(m) : 0u;
            m &= m - 1;
        }
        if (five) {
            bool sv = false;
            const uint64_t alt = idx_alt_longest(f + t[3] + 1, t[4] - t[3] - 1, &sv);
            if (!sv) {
                done = true;
                const uint32_t have = (uint32_t)vw::popc64(m);
                if (have < 3 && !idx_more_tabs(in, rs + 8 + IS_WIN, re, 3 - have)) code = 3;
                else if (!idx_strtoul(f + t[0] + 1, t[1] - t[0] - 1, &pos)) code = 2;
                else {
                    ref = idx_ref(f, t[0]);
                    const uint64_t rl = t[3] - t[2] - 1;
                    end = pos + (rl >= alt ? rl : alt) - 1;
                }
            }
        }
    }
    if (!done) code = idx_span_seq(in, rs, re, &ref, &pos, &end);
    ref_idx[i] = (uint8_t)ref;
    pos_out[i] = pos;
    end_out[i] = end;
    if (code) atomicMin((unsigned long long *)err, (unsigned long long)((i << 8) | code));
}

// ---------------------------------------------------------------------------
// Inclusive unsigned 64-bit prefix maximum (identity 0).

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// value of lane l - d (0 for the first d lanes): two 32-bit lane gathers
__device__ __forceinline__ uint64_t lane_up64(uint64_t v, uint32_t l, uint32_t d) {
    const uint32_t src = (l - d) & 63u;
    const uint32_t lo = vw::shfl((uint32_t)v, src), hi = vw::shfl((uint32_t)(v >> 32), src);
    return l >= d ? ((uint64_t)hi << 32) | lo : 0ull;
}

__device__ __forceinline__ uint64_t wave_scan_max64(uint64_t v, uint32_t l) {
    for (uint32_t d = 1; d < 64; d <<= 1) v = umax64(v, lane_up64(v, l, d));
    return v;
}

// Block scan over 256 threads (all of them call it): returns the maximum of
// the values before this thread in the block, *total = the block's maximum.
__device__ uint64_t block_excl_max64(uint64_t v, uint64_t *sh, uint64_t *total) {
    const uint32_t l = vw::lane_id(), w = threadIdx.x >> 6;
    const uint64_t inc = wave_scan_max64(v, l);
    const uint64_t prev = lane_up64(inc, l, 1);
    if (l == 63u) sh[w] = inc;
    __syncthreads();
    const uint64_t t0 = sh[0], t1 = sh[1], t2 = sh[2], t3 = sh[3];
    __syncthreads();   // (sh is reused by the caller's next scan)
    *total = umax64(umax64(t0, t1), umax64(t2, t3));
    const uint64_t before = umax64(umax64(w > 0 ? t0 : 0, w > 1 ? t1 : 0), w > 2 ? t2 : 0);
    return umax64(before, prev);
}

__global__ __launch_bounds__(256) void k_idx_blockmax(const uint64_t *end, uint64_t n, uint64_t *bmax) {
    __shared__ uint64_t sh[4];
    const uint64_t i = (uint64_t)blockIdx.x * IDX_THREADS + threadIdx.x;
    uint64_t tot;
    block_excl_max64(i < n ? end[i] : 0, sh, &tot);
    if (threadIdx.x == 0) bmax[blockIdx.x] = tot;
}

// in place: bmax[b] = maximum of the blocks before b (one block)
__global__ __launch_bounds__(256) void k_idx_partials(uint64_t *bmax, uint64_t nb) {
    __shared__ uint64_t sh[4];
    uint64_t carry = 0;
    for (uint64_t b = 0; b < nb; b += IDX_THREADS) {
        const uint64_t i = b + threadIdx.x;
        uint64_t tot;
        const uint64_t e = block_excl_max64(i < nb ? bmax[i] : 0, sh, &tot);
        if (i < nb) bmax[i] = umax64(carry, e);
        carry = umax64(carry, tot);
    }
}

// M_i = prefix maximum of end; record i opens an entry iff i == 0, or
// i % E == 0 and end_i > M_{i-1}
__global__ __launch_bounds__(256) void k_idx_flags(const uint64_t *end, uint64_t n, const uint64_t *bmax, uint64_t E,
                                                   uint64_t *pmax, uint32_t *flag) {
    __shared__ uint64_t sh[4];
    const uint64_t i = (uint64_t)blockIdx.x * IDX_THREADS + threadIdx.x;
    const uint64_t v = i < n ? end[i] : 0;
    uint64_t tot;
    const uint64_t before = umax64(bmax[blockIdx.x], block_excl_max64(v, sh, &tot));
    if (i < n) {
        pmax[i] = umax64(before, v);
        flag[i] = (i == 0 || (i % E == 0 && v > before)) ? 1u : 0u;
    }
}

// Entry j, opened at record k_j: {ref_idx[k_j], (u32)M_{k_{j+1}-1}, base +
// rec[k_j]}, 13 packed bytes.  The opening record stores bytes 0 and 5..12,
// the entry's last record bytes 1..4; the last record also stores the count
// and the largest end.
__global__ __launch_bounds__(256) void k_idx_emit(const uint8_t *ref_idx, const uint64_t *rec, const uint64_t *pmax,
                                                  const uint32_t *flag, const uint64_t *eno, uint64_t n,
                                                  uint64_t base, uint8_t *entries, uint64_t cap, uint64_t *count,
                                                  uint64_t *info, uint64_t *err) {
    const uint64_t i = (uint64_t)blockIdx.x * IDX_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t fl = flag[i];
    const uint64_t j = eno[i];
    if (fl) {
        if (j < cap) {
            uint8_t *e = entries + 13 * j;
            const uint64_t off = base + rec[i];
            e[0] = ref_idx[i];
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) e[5 + k] = (uint8_t)(off >> (8 * k));
        } else {
            atomicMin((unsigned long long *)err, (unsigned long long)((i << 8) | 0xFFu));
        }
    }
    const bool last = i + 1 == n;
    if (last || flag[i + 1]) {
        const uint64_t jj = j + fl - 1;   // the entry this record belongs to (record 0 always opens one)
        const uint64_t m = pmax[i];
        if (jj < cap) {
            uint8_t *e = entries + 13 * jj;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) e[1 + k] = (uint8_t)(m >> (8 * k));
        }
        if (last) {
            *count = j + fl;
            *info = m;
        }
    }
}

// words of one call: err = ~0 (a, nullable), b = vb (nullable), c = vc (nullable)
__global__ void k_idx_reset(uint64_t *a, uint64_t *b, uint64_t vb, uint64_t *c, uint64_t vc) {
    if (threadIdx.x == 0) {
        if (a) *a = ~0ull;
        if (b) *b = vb;
        if (c) *c = vc;
    }
}

// compare_to_range (src/main.cpp:110-137) of record i against the query:
// before (skipped), after (the walk stops), else selected
__global__ __launch_bounds__(256) void k_index_compare(const uint8_t *ref_idx, const uint64_t *pos,
                                                       const uint64_t *end, uint64_t n, uint32_t qidx, uint64_t qstart,
                                                       uint64_t qend, uint8_t *flag, uint64_t *first_after) {
    const uint64_t i = (uint64_t)blockIdx.x * IDX_THREADS + threadIdx.x;
    bool after = false;
    if (i < n) {
        const uint32_t idx = ref_idx[i];
        const bool before = idx < qidx || (idx == qidx && end[i] < qstart);
        after = !before && (idx > qidx || (idx == qidx && pos[i] > qend));
        flag[i] = (!before && !after) ? 1 : 0;
    }
    // one atomic per wave: its lowest "after" lane
    const uint64_t m = vw::ballot(after);
    if (after && vw::lane_id() == (uint32_t)__builtin_ctzll(m))
        atomicMin((unsigned long long *)first_after, (unsigned long long)i);
}

}  // namespace

VcfcIndexLayout vcfc_index_workspace_layout(uint64_t n) {
    auto al = [](uint64_t x) { return (x + 255) & ~255ull; };
    VcfcIndexLayout L;
    uint64_t o = 0;
    L.ref_idx = o; o = al(o + n + 1);
    L.pos = o; o = al(o + 8 * (n + 1));
    L.end = o; o = al(o + 8 * (n + 1));
    L.pmax = o; o = al(o + 8 * (n + 1));
    L.flag = o; o = al(o + 4 * (n + 1));
    L.eno = o; o = al(o + 8 * (n + 1));
    L.bmax = o; o = al(o + 8 * ((n + IDX_THREADS - 1) / IDX_THREADS + 1));
    L.partials = o; o = al(o + 8 * ((n + 4095) / 4096 + 1));
    L.total = o;
    return L;
}

hipError_t vcfc_index_span(const uint8_t *in, const uint64_t *rec_start, uint64_t n, uint8_t *ref_idx, uint64_t *pos,
                           uint64_t *end, uint64_t *err, hipStream_t s) {
    hipLaunchKernelGGL(k_idx_reset, dim3(1), dim3(64), 0, s, err, (uint64_t *)nullptr, 0ull, (uint64_t *)nullptr, 0ull);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    const dim3 grid((unsigned)((n + IDX_THREADS - 1) / IDX_THREADS));
    hipLaunchKernelGGL(k_index_span, grid, dim3(IDX_THREADS), 0, s, in, rec_start, n, ref_idx, pos, end, err);
    return hipGetLastError();
}

hipError_t vcfc_index_build(const uint8_t *in, const uint64_t *rec_start, uint64_t n, uint64_t base_offset,
                            uint64_t entries_per_bin, uint8_t *entries, uint64_t entries_cap, uint64_t *count,
                            uint64_t *info, uint8_t *ws, const VcfcIndexLayout &L, uint64_t *err, hipStream_t s) {
    uint8_t *ref_idx = ws + L.ref_idx;
    uint64_t *pos = reinterpret_cast<uint64_t *>(ws + L.pos), *end = reinterpret_cast<uint64_t *>(ws + L.end);
    uint64_t *pmax = reinterpret_cast<uint64_t *>(ws + L.pmax), *eno = reinterpret_cast<uint64_t *>(ws + L.eno);
    uint64_t *bmax = reinterpret_cast<uint64_t *>(ws + L.bmax), *part = reinterpret_cast<uint64_t *>(ws + L.partials);
    uint32_t *flag = reinterpret_cast<uint32_t *>(ws + L.flag);
    hipLaunchKernelGGL(k_idx_reset, dim3(1), dim3(64), 0, s, err, count, 0ull, info, 0ull);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    const uint64_t nb = (n + IDX_THREADS - 1) / IDX_THREADS;
    const dim3 grid((unsigned)nb), block(IDX_THREADS);
    hipLaunchKernelGGL(k_index_span, grid, block, 0, s, in, rec_start, n, ref_idx, pos, end, err);
    hipLaunchKernelGGL(k_idx_blockmax, grid, block, 0, s, (const uint64_t *)end, n, bmax);
    hipLaunchKernelGGL(k_idx_partials, dim3(1), block, 0, s, bmax, nb);
    hipLaunchKernelGGL(k_idx_flags, grid, block, 0, s, (const uint64_t *)end, n, (const uint64_t *)bmax,
                       entries_per_bin, pmax, flag);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = vcfc_scan_u32(flag, n, part, eno, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_idx_emit, grid, block, 0, s, (const uint8_t *)ref_idx, rec_start, (const uint64_t *)pmax,
                       (const uint32_t *)flag, (const uint64_t *)eno, n, base_offset, entries, entries_cap, count,
                       info, err);
    return hipGetLastError();
}

hipError_t vcfc_index_compare(const uint8_t *ref_idx, const uint64_t *pos, const uint64_t *end, uint64_t n,
                              uint32_t qidx, uint64_t qstart, uint64_t qend, uint8_t *flag, uint64_t *first_after,
                              hipStream_t s) {
    hipLaunchKernelGGL(k_idx_reset, dim3(1), dim3(64), 0, s, first_after, (uint64_t *)nullptr, 0ull,
                       (uint64_t *)nullptr, 0ull);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    const dim3 grid((unsigned)((n + IDX_THREADS - 1) / IDX_THREADS));
    hipLaunchKernelGGL(k_index_compare, grid, dim3(IDX_THREADS), 0, s, ref_idx, pos, end, n, qidx, qstart, qend, flag,
                       first_after);
    return hipGetLastError();
}
