// vcfc_ld.hip -- gfx950 kernels of ld-window: for every pair
// of .bed rows (i, i + k), k = 1..W, the 3 x 3 table of the samples' genotypes
// (both called), nine uint32 at slot i * W + k - 1.
//
//   k_ld_reset    the call's state: the row count (read on the device), the
//                 rows whose W slots all lie inside pairs_cap, and the error
//                 word where no matrix call set it; a short pairs_cap is
//                 reported (code 0xFF) here, or by k_ld_cap at its record.
//   k_ld_planes   a .bed row (2 bits a sample: 11 g = 0, 10 g = 1, 00 g = 2,
//                 01 missing) as three bit planes, 32 samples a word: H
//                 (g = 1), B (g = 2), V (called).  Compacted, not left spread
//                 at 16 samples a word: the pair kernel's work is one AND and
//                 one population count per plane word, so half the words is
//                 half the work, and the compaction is paid once a row where
//                 the words are read W times.  Columns >= S and the words up
//                 to the plane stride are 0 in all three.
//   k_ld_pairs    a block owns VCFC_LD_TILE_ROWS rows i and up to
//                 VCFC_LD_TILE_PARTNERS partners k (blockIdx.y: the partner
//                 tile); a lane owns pairs.  The planes of the rows i and of
//                 the partner rows go through LDS in chunks of
//                 VCFC_LD_CHUNK_SAMPLES samples (S is unbounded: a longer row
//                 loops), a row that does not exist as zeros.  An LDS row is
//                 3 * 16 + 1 words: the lanes of a wave read consecutive
//                 partner rows, which an odd pitch spreads over the banks,
//                 and the lanes that share a row i read one address.  Nine
//                 AND + population counts per plane word: the four cells of
//                 g in {1, 2} and the marginals against V; the other five
//                 cells by subtraction.  The tables leave through LDS as the
//                 contiguous dword stream their slots form.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vcfc_wave.h>   // angle brackets: tests/simt_emu shadows it
#include "vcfc_bed_planes.h"
#include "vcfc_device.h"

namespace {

constexpr uint32_t LD_R = VCFC_LD_TILE_ROWS;
constexpr uint32_t LD_KT = VCFC_LD_TILE_PARTNERS;
constexpr uint32_t LD_CH = VCFC_LD_CHUNK_SAMPLES / 32;   // plane words of a row in LDS at a time
constexpr uint32_t LD_PITCH = 3 * LD_CH + 1;             // odd: consecutive rows on different banks
constexpr uint32_t LD_JROWS = LD_R + LD_KT - 1;          // partner rows of a tile
constexpr uint32_t LD_THREADS = 256;
constexpr uint32_t LD_PPT = LD_R * LD_KT / LD_THREADS;   // pairs a lane owns at most
static_assert(LD_CH % 4 == 0 && LD_R * LD_KT % LD_THREADS == 0, "the staging loads 16 bytes; whole passes");

__device__ __forceinline__ uint32_t ld_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

__global__ void k_ld_reset(VcfcLdArgs a) {
    if (threadIdx.x != 0) return;
    const uint64_t rows = a.rows_dev ? *a.rows_dev : a.n;
    const uint64_t fit = std::min<uint64_t>(rows, a.pairs_cap / a.W);
    a.state[0] = rows;
    a.state[1] = fit;
    if (a.own_err) *a.err = fit < rows ? ((fit << 8) | 0xFFull) : ~0ull;
}

// the composed call: the first record whose row's slots do not all fit
__global__ __launch_bounds__(256) void k_ld_cap(VcfcLdArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n || a.state[1] == a.state[0] || (a.select && !a.select[i])) return;
    if (a.row_of[i] >= a.state[1]) atomicMin((unsigned long long *)a.err, (unsigned long long)((i << 8) | 0xFFull));
}

// One lane per plane word (vcfc_bed::word_planes: the 8 row bytes of its 32
// samples).
__global__ __launch_bounds__(256) void k_ld_planes(VcfcLdArgs a) {
    const uint64_t rows = a.state[0], P = a.plane_words;
    const uint32_t S = (uint32_t)a.S, rb = (S + 3u) >> 2, nw = (S + 31u) >> 5;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < rows * P; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = e / P;
        const uint32_t w = (uint32_t)(e % P);
        uint32_t H = 0, B = 0, V = 0;
        if (w < nw) {
            vcfc_bed::word_planes(a.bed + r * a.row_stride + 8ull * w, w, S, rb, H, B, V);
        }
        uint32_t *o = a.planes + 3ull * r * P + w;
        o[0] = H;
        o[P] = B;
        o[2 * P] = V;
    }
}

// rows [r0, r0 + nr) of the planes, words [c0, c0 + LD_CH), into t (row pitch
// LD_PITCH, the three planes LD_CH apart); a row >= rows and a word >= P as 0
__device__ __forceinline__ void ld_stage(const VcfcLdArgs &a, uint32_t *t, uint64_t r0, uint32_t nr, uint32_t c0, uint64_t rows) {
    const uint32_t P = (uint32_t)a.plane_words;
    for (uint32_t e = threadIdx.x; e < nr * 3u * (LD_CH / 4u); e += LD_THREADS) {
        const uint32_t rl = e / (3u * (LD_CH / 4u)), rem = e % (3u * (LD_CH / 4u));
        const uint32_t pl = rem / (LD_CH / 4u), w = 4u * (rem % (LD_CH / 4u));
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (r0 + rl < rows && c0 + w < P)
            v = *reinterpret_cast<const uint4 *>(a.planes + (3ull * (r0 + rl) + pl) * P + c0 + w);
        uint32_t *d = t + rl * LD_PITCH + pl * LD_CH + w;
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
}

__global__ __launch_bounds__(LD_THREADS) void k_ld_pairs(VcfcLdArgs a) {
    __shared__ uint32_t it[LD_R * LD_PITCH];
    __shared__ uint32_t jt[LD_JROWS * LD_PITCH];
    __shared__ uint32_t ot[LD_THREADS * 9];
    const uint64_t rows = a.state[0], fit = a.state[1];
    const uint64_t i0 = (uint64_t)blockIdx.x * LD_R;
    if (i0 >= fit) return;   // (the whole block)
    const uint32_t W = (uint32_t)a.W, kte = ld_min(W, LD_KT), k0 = blockIdx.y * LD_KT;
    const uint32_t npairs = LD_R * kte, tid = threadIdx.x;
    const uint32_t nw = ((uint32_t)a.S + 31u) >> 5;
    // pair q of the tile: row i0 + q / kte, partner k0 + q % kte + 1
    uint32_t xo[LD_PPT], yo[LD_PPT], acc[LD_PPT][9];
#pragma unroll
    for (uint32_t p = 0; p < LD_PPT; p++) {
        const uint32_t q = ld_min(tid + LD_THREADS * p, npairs - 1u);
        xo[p] = (q / kte) * LD_PITCH;
        yo[p] = (q / kte + q % kte) * LD_PITCH;
#pragma unroll
        for (uint32_t e = 0; e < 9; e++) acc[p][e] = 0;
    }
    for (uint32_t c0 = 0; c0 < nw; c0 += LD_CH) {
        __syncthreads();   // the previous chunk has been read
        ld_stage(a, it, i0, LD_R, c0, rows);
        ld_stage(a, jt, i0 + k0 + 1u, LD_R + kte - 1u, c0, rows);
        __syncthreads();
        const uint32_t cw = ld_min(LD_CH, nw - c0);
#pragma unroll
        for (uint32_t p = 0; p < LD_PPT; p++) {
            if (LD_THREADS * p >= npairs) break;   // (the whole block)
            const uint32_t *x = it + xo[p], *y = jt + yo[p];
            for (uint32_t w = 0; w < cw; w++) {
                const uint32_t hi = x[w], bi = x[LD_CH + w], vi = x[2 * LD_CH + w];
                const uint32_t hj = y[w], bj = y[LD_CH + w], vj = y[2 * LD_CH + w];
                acc[p][0] += __builtin_popcount(hi & hj);
                acc[p][1] += __builtin_popcount(hi & bj);
                acc[p][2] += __builtin_popcount(bi & hj);
                acc[p][3] += __builtin_popcount(bi & bj);
                acc[p][4] += __builtin_popcount(hi & vj);
                acc[p][5] += __builtin_popcount(bi & vj);
                acc[p][6] += __builtin_popcount(vi & hj);
                acc[p][7] += __builtin_popcount(vi & bj);
                acc[p][8] += __builtin_popcount(vi & vj);
            }
        }
    }
    // a pass's 256 tables through LDS, then out as consecutive dwords
    const uint64_t own = std::min<uint64_t>(LD_R, fit - i0);   // rows of the tile that are written
#pragma unroll
    for (uint32_t p = 0; p < LD_PPT; p++) {
        if (LD_THREADS * p >= npairs) break;   // (the whole block)
        const uint32_t n11 = acc[p][0], n12 = acc[p][1], n21 = acc[p][2], n22 = acc[p][3];
        const uint32_t r1 = acc[p][4], r2 = acc[p][5], c1 = acc[p][6], c2 = acc[p][7], N = acc[p][8];
        __syncthreads();   // the previous pass has left ot
        uint32_t *o = ot + 9u * tid;
        o[0] = N - r1 - r2 - c1 - c2 + n11 + n12 + n21 + n22;
        o[1] = c1 - n11 - n21;
        o[2] = c2 - n12 - n22;
        o[3] = r1 - n11 - n12;
        o[4] = n11;
        o[5] = n12;
        o[6] = r2 - n21 - n22;
        o[7] = n21;
        o[8] = n22;
        __syncthreads();
        for (uint32_t d = tid; d < 9u * LD_THREADS; d += LD_THREADS) {
            const uint32_t q = LD_THREADS * p + d / 9u;
            if (q >= npairs) break;
            const uint32_t il = q / kte, kk = q % kte;
            if (il >= own || k0 + kk >= W) continue;
            a.tables[((i0 + il) * W + k0 + kk) * 9ull + d % 9u] = ot[d];
        }
    }
}

}  // namespace

VcfcLdLayout vcfc_ld_workspace_layout(uint64_t n, uint64_t S) {
    auto al = [](uint64_t x) { return (x + 255) & ~255ull; };
    VcfcLdLayout L;
    L.plane_words = (((S + 31) / 32) + 3) & ~3ull;
    L.bed_stride = (vcfc_matrix_row_size(VCFC_MATRIX_BED, S) + 15) & ~15ull;
    uint64_t o = 0;
    L.state = o; o = al(o + 16);
    L.planes = o; o = al(o + 12 * L.plane_words * n);
    L.bed = o; o = al(o + L.bed_stride * n + 64);
    L.matrix = o; o = al(o + vcfc_matrix_workspace_layout(n).total);
    L.total = o;
    return L;
}

hipError_t vcfc_ld_run(const VcfcLdArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_ld_reset, dim3(1), dim3(64), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.n == 0) return e;
    if (a.rows_dev) {
        hipLaunchKernelGGL(k_ld_cap, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const uint64_t want = (a.n * a.plane_words + 255) / 256;
    hipLaunchKernelGGL(k_ld_planes, dim3((unsigned)std::min<uint64_t>(want, 1u << 20)), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 grid((unsigned)((a.n + LD_R - 1) / LD_R), (unsigned)((a.W + LD_KT - 1) / LD_KT));
    hipLaunchKernelGGL(k_ld_pairs, grid, dim3(LD_THREADS), 0, s, a);
    return hipGetLastError();
}
