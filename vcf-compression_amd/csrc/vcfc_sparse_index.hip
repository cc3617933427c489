// vcfc_sparse_index.hip -- gfx950 kernels of the sparse external index
// (create-sparse-index / query-sparse-index; reference
// create_sparse_external_index, src/main.cpp:854-999,
// query_sparse_external_index :1002-1281, compute_sparse_offset,
// src/sparse.cpp:18-51).
//
//   k_sparse_span<false>  one lane per record: ref_idx and POS under create's
//                         field rules (five TABs; eight and the INFO walk of
//                         compute_end_position only for a structural ALT)
//   k_sparse_span<true>   the query walk's rules: CHROM and POS only
//   k_sparse_resolve      the slot offset of every record, keep[i] = the last
//                         record of a run of equal offsets, the out-of-order
//                         flag and the first offset that lseek refuses
//   (vcfc_scan_u32        entry number of every kept record)
//   k_sparse_emit         the kept 13-byte entries and their offsets, densely
//   k_gap_fields          gap-analysis (:3931-3980): each record's POS text
//                         location and the reference's compressed count
//
// Every cross-lane step uses csrc/vcfc_wave.h only, so tests/simt_emu runs
// this file on the CPU.
#include <hip/hip_runtime.h>
#include <vcfc_wave.h>   // angle brackets: tests/simt_emu shadows it
#include "vcfc_device.h"
#include "vcfc_decode_dev.h"   // be30

namespace {

constexpr uint32_t SPX_THREADS = 256;

#include "vcfc_index_dev.h"

// Byte-serial form for the record in[rs, re): 0, or code 2 / 3.  The POS
// parse comes before the later TABs, as in the reference (:919-925).
template <bool WALK>
__device__ uint32_t spx_span_seq(const uint8_t *in, uint64_t rs, uint64_t re, uint32_t *ref, uint64_t *pos) {
    uint64_t t[8];
    uint64_t k = rs + 8;
    for (uint32_t f = 0; f < 2; f++) {
        while (k < re && in[k] != '\t') k++;
        if (k >= re) return 3;
        t[f] = k++;
    }
    *ref = idx_ref(in + rs + 8, t[0] - (rs + 8));
    if (!idx_strtoul(in + t[0] + 1, t[1] - t[0] - 1, pos)) return 2;
    if (WALK) return 0;
    for (uint32_t f = 2; f < 5; f++) {
        while (k < re && in[k] != '\t') k++;
        if (k >= re) return 3;
        t[f] = k++;
    }
    bool sv = false;
    for (uint64_t a = t[3] + 1; a < t[4]; a++) sv = sv || in[a] == '<';
    if (!sv) return 0;
    for (uint32_t f = 5; f < 8; f++) {
        while (k < re && in[k] != '\t') k++;
        if (k >= re) return 3;
        t[f] = k++;
    }
    uint64_t end = 0;   // unused by the reference too (:946); only its throws count
    return idx_sv_end(in + t[6] + 1, t[7] - t[6] - 1, *pos, &end) ? 0u : 2u;
}

// One lane per record.  Fast path: the 48 bytes from the CHROM start lie
// inside the record and hold the TABs this action reads (two for the walk;
// five for create, with an ALT that holds no '<'): three 16-byte loads, the
// TABs found by SWAR in registers, CHROM and POS parsed from an LDS copy.
// Nothing after ALT is read.  Otherwise byte by byte.
constexpr uint32_t SPX_WIN = 48;
template <bool WALK>
__global__ __launch_bounds__(256) void k_sparse_span(const uint8_t *in, const uint64_t *rec, uint64_t n,
                                                     uint8_t *ref_idx, uint64_t *pos_out, uint64_t *err) {
    __shared__ __attribute__((aligned(16))) uint8_t win[SPX_THREADS * SPX_WIN];
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t rs = rec[i], re = rec[i + 1];
    uint32_t ref = 0, code = 0;
    uint64_t pos = 0;
    bool done = false;
    if (re >= rs + 8 + SPX_WIN) {
        const uint8_t *p = in + rs + 8;
        const uint4 v0 = vw::uload16(p), v1 = vw::uload16(p + 16), v2 = vw::uload16(p + 32);
        uint8_t *f = win + threadIdx.x * SPX_WIN;
        uint4 *w = reinterpret_cast<uint4 *>(f);
        w[0] = v0; w[1] = v1; w[2] = v2;
        uint64_t m = tab_bits16(v0) | tab_bits16(v1) << 16 | tab_bits16(v2) << 32;
        constexpr uint32_t NEED = WALK ? 2 : 5;
        uint32_t t[NEED];
        bool all = true;
#pragma unroll
        for (uint32_t k = 0; k < NEED; k++) {
            all = all && m != 0;
            t[k] = m ? (uint32_t)__builtin_ctzll(m) : 0u;
            m &= m - 1;
        }
        if (all) {
            bool sv = false;
            if constexpr (!WALK)
                for (uint32_t a = t[3] + 1; a < t[4]; a++) sv = sv || f[a] == '<';
            if (!sv) {
                done = true;
                ref = idx_ref(f, t[0]);
                if (!idx_strtoul(f + t[0] + 1, t[1] - t[0] - 1, &pos)) code = 2;
            }
        }
    }
    if (!done) code = spx_span_seq<WALK>(in, rs, re, &ref, &pos);
    ref_idx[i] = (uint8_t)ref;
    pos_out[i] = pos;
    if (code) atomicMin((unsigned long long *)err, (unsigned long long)((i << 8) | code));
}

// (300000000 + pos) * 256 in 64-bit wrap-around arithmetic
// (compute_sparse_offset with multiplication_factor 1, block_size 256 and
// VCFC_SPARSE_MULTIPLE_REF_PER_FILE false)
__device__ __forceinline__ uint64_t spx_off(uint64_t pos) { return (300000000ull + pos) * 256ull; }

// Equal offsets are adjacent while the offsets do not decrease; then the last
// record of each run is the one the reference's sequential writes leave.
// status[1] = 1 where some offset decreases (the host then writes every entry
// in record order), status[2] = the first record whose offset is negative as
// off_t (lseek fails there).  One atomic per wave for each.
__global__ __launch_bounds__(256) void k_sparse_resolve(const uint64_t *pos, uint64_t n, uint64_t *off,
                                                        uint32_t *keep, uint64_t *status) {
    const uint64_t i = (uint64_t)blockIdx.x * SPX_THREADS + threadIdx.x;
    bool down = false, neg = false;
    if (i < n) {
        const uint64_t o = spx_off(pos[i]);
        const bool last = i + 1 == n;
        const uint64_t o1 = last ? 0 : spx_off(pos[i + 1]);
        off[i] = o;
        keep[i] = (last || o != o1) ? 1u : 0u;
        down = !last && o1 < o;
        neg = (int64_t)o < 0;
    }
    const uint32_t l = vw::lane_id();
    const uint64_t md = vw::ballot(down), mn = vw::ballot(neg);
    if (down && l == (uint32_t)__builtin_ctzll(md)) atomicMax((unsigned long long *)(status + 1), 1ull);
    if (neg && l == (uint32_t)__builtin_ctzll(mn)) atomicMin((unsigned long long *)(status + 2), (unsigned long long)i);
}

// The kept record i is entry j = eno[i]: {ref_idx, (u32)pos, base + rec[i]},
// 13 packed little-endian bytes, and its file offset.
__global__ __launch_bounds__(256) void k_sparse_emit(const uint8_t *ref_idx, const uint64_t *pos, const uint64_t *off,
                                                     const uint64_t *rec, const uint32_t *keep, const uint64_t *eno,
                                                     uint64_t n, uint64_t base, uint8_t *entries, uint64_t *file_off,
                                                     uint64_t *count) {
    const uint64_t i = (uint64_t)blockIdx.x * SPX_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t j = eno[i];
    if (keep[i]) {   // j < n: the caller's arrays hold n entries
        uint8_t *e = entries + 13 * j;
        const uint64_t p = pos[i], bo = base + rec[i];
        e[0] = ref_idx[i];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) e[1 + k] = (uint8_t)(p >> (8 * k));
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) e[5 + k] = (uint8_t)(bo >> (8 * k));
        file_off[j] = off[i];
    }
    if (i + 1 == n) *count = j + 1;   // the last record is always kept
}

// gap-analysis (reference src/main.cpp:3931-3980), one lane per record: where
// the line's POS text lies -- the second non-empty TAB field, which the
// required columns hold verbatim -- and the reference's compressed count
// (line_byte_count, src/compress.cpp:764-968): the 8 header bytes, the
// required columns and every sample-section byte it reads, where the closing
// LF counts only when it ends an uncompressed column (:880-891; the LF read
// at :958 is not counted).  The walk is dec_line_seq's (vcfc_decode.hip)
// without its output; the exact decode plan validates the same records, so a
// record refused here (code 3) is refused there too, except one whose second
// non-empty field does not lie wholly in its required columns: fewer than two
// such fields there, or the second one ended by the columns' end with sample
// tokens after it (the line's field then runs on into the first token).
__global__ __launch_bounds__(256) void k_gap_fields(const uint8_t *in, const uint64_t *rec, uint64_t n, uint64_t S,
                                                    uint64_t *pos_off, uint32_t *pos_len, uint64_t *ccount,
                                                    uint64_t *err) {
    const uint64_t i = (uint64_t)blockIdx.x * SPX_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t rs = rec[i], re = rec[i + 1];
    uint64_t po = 0, cnt = 0;
    uint32_t pl = 0;
    bool ok = re - rs > 8;
    uint64_t s0 = re;
    if (ok) {
        const uint64_t req = be30(in + rs + 4);
        s0 = rs + 8 + req;
        ok = req > 0 && s0 < re;
        cnt = 8 + req;
    }
    if (ok) {
        uint32_t found = 0;
        uint64_t fs = rs + 8;
        for (uint64_t k = rs + 8; k <= s0 && found < 2; k++) {
            if (k == s0 ? S == 0 : in[k] == '\t') {
                if (k > fs && ++found == 2) { po = fs; pl = (uint32_t)(k - fs); }
                fs = k + 1;
            }
        }
        ok = found == 2;
    }
    if (ok) {
        uint64_t ip = s0, got = 0;
        while (ok && got < S) {
            if (ip >= re) { ok = false; break; }
            const uint8_t b = in[ip++];
            cnt++;
            if ((b & 0x80u) == 0) {
                got += b;
            } else if ((b & 0xE0u) == 0xE0u) {
                const uint32_t uc = b & 0x1Fu;
                uint32_t u = 0;
                while (u < uc) {
                    if (ip >= re) { ok = false; break; }
                    const uint8_t x = in[ip++];
                    cnt++;
                    if (x == '\n') {
                        u++; got++;
                        ip--;   // read again as the line end, uncounted
                        if (u != uc) { ok = false; break; }
                    } else if (x == '\t') {
                        u++; got++;
                    }
                }
            } else {
                got += b & 0x1Fu;
            }
        }
    }
    pos_off[i] = po;
    pos_len[i] = pl;
    ccount[i] = cnt;
    if (!ok) atomicMin((unsigned long long *)err, (unsigned long long)((i << 8) | 3u));
}

// the words of one call: *err = ~0, *count = 0, status = {0, 0, ~0} (each nullable)
__global__ void k_sparse_reset(uint64_t *err, uint64_t *count, uint64_t *status) {
    if (threadIdx.x == 0) {
        if (err) *err = ~0ull;
        if (count) *count = 0;
        if (status) { status[0] = 0; status[1] = 0; status[2] = ~0ull; }
    }
}

}  // namespace

VcfcSparseIndexLayout vcfc_sparse_index_workspace_layout(uint64_t n) {
    auto al = [](uint64_t x) { return (x + 255) & ~255ull; };
    VcfcSparseIndexLayout L;
    uint64_t o = 0;
    L.ref_idx = o; o = al(o + n + 1);
    L.pos = o; o = al(o + 8 * (n + 1));
    L.off = o; o = al(o + 8 * (n + 1));
    L.keep = o; o = al(o + 4 * (n + 1));
    L.eno = o; o = al(o + 8 * (n + 1));
    L.partials = o; o = al(o + 8 * ((n + 4095) / 4096 + 1));
    L.total = o;
    return L;
}

hipError_t vcfc_sparse_index_span(const uint8_t *in, const uint64_t *rec_start, uint64_t n, int walk, uint8_t *ref_idx,
                                  uint64_t *pos, uint64_t *err, hipStream_t s) {
    hipLaunchKernelGGL(k_sparse_reset, dim3(1), dim3(64), 0, s, err, (uint64_t *)nullptr, (uint64_t *)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    const dim3 grid((unsigned)((n + SPX_THREADS - 1) / SPX_THREADS)), block(SPX_THREADS);
    if (walk) hipLaunchKernelGGL(k_sparse_span<true>, grid, block, 0, s, in, rec_start, n, ref_idx, pos, err);
    else hipLaunchKernelGGL(k_sparse_span<false>, grid, block, 0, s, in, rec_start, n, ref_idx, pos, err);
    return hipGetLastError();
}

hipError_t vcfc_sparse_index_build(const uint8_t *in, const uint64_t *rec_start, uint64_t n, uint64_t base_offset,
                                   uint8_t *entries, uint64_t *file_off, uint64_t *count, uint64_t *status,
                                   uint8_t *ws, const VcfcSparseIndexLayout &L, uint64_t *err, hipStream_t s) {
    uint8_t *ref_idx = ws + L.ref_idx;
    uint64_t *pos = reinterpret_cast<uint64_t *>(ws + L.pos), *off = reinterpret_cast<uint64_t *>(ws + L.off);
    uint64_t *eno = reinterpret_cast<uint64_t *>(ws + L.eno), *part = reinterpret_cast<uint64_t *>(ws + L.partials);
    uint32_t *keep = reinterpret_cast<uint32_t *>(ws + L.keep);
    hipLaunchKernelGGL(k_sparse_reset, dim3(1), dim3(64), 0, s, err, count, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    const dim3 grid((unsigned)((n + SPX_THREADS - 1) / SPX_THREADS)), block(SPX_THREADS);
    hipLaunchKernelGGL(k_sparse_span<false>, grid, block, 0, s, in, rec_start, n, ref_idx, pos, err);
    hipLaunchKernelGGL(k_sparse_resolve, grid, block, 0, s, (const uint64_t *)pos, n, off, keep, status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = vcfc_scan_u32(keep, n, part, eno, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sparse_emit, grid, block, 0, s, (const uint8_t *)ref_idx, (const uint64_t *)pos,
                       (const uint64_t *)off, rec_start, (const uint32_t *)keep, (const uint64_t *)eno, n, base_offset,
                       entries, file_off, count);
    return hipGetLastError();
}

hipError_t vcfc_gap_fields(const uint8_t *in, const uint64_t *rec_start, uint64_t n, uint64_t S, uint64_t *pos_off,
                           uint32_t *pos_len, uint64_t *ccount, uint64_t *err, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + SPX_THREADS - 1) / SPX_THREADS)), block(SPX_THREADS);
    hipLaunchKernelGGL(k_gap_fields, grid, block, 0, s, in, rec_start, n, S, pos_off, pos_len, ccount, err);
    return hipGetLastError();
}
