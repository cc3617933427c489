// vcfc_kin.hip -- gfx950 kernels of kinship: for every pair of
// samples (i, j) the 3 x 3 table of their genotypes over the .bed rows (both
// called), nine uint32 at (i * S + j) * 9: the full square.
//
//   k_kin_reset   the call's state: the rows that are counted -- n, or in the
//                 composed call row_of[n], cut to row_of[k] where the matrix
//                 call's error word holds (k << 8 | 3), so the tables are those
//                 of the rows before the failing record --, and the error word
//                 where no matrix call set it.
//   k_kin_planes  .bed rows (variant-major, 2 bits a sample) as sample-major
//                 bit planes H (g = 1), B (g = 2), V (called), 32 variants a
//                 word.  A lane holds one row's word of 32 samples of each
//                 plane (vcfc_bed::word_planes, as k_ld_planes);
//                 ballot((H >> b) & 1) is then sample b's 64 variants of the
//                 wave's 64 rows.  A block covers VCFC_KIN_PLANE_ROWS rows
//                 (four waves) and four sample words: the ballots meet in LDS
//                 and leave as 32 contiguous bytes a sample and plane, and a
//                 lane's four loads cover 32 contiguous bytes of its row.
//                 Rows at or past the count are zeros, up to row_words.
//   k_kin_pairs   a block owns a tile of 32 x 32 sample pairs (ti <= tj only),
//                 a lane a 2 x 2 block of them: samples ly, ly + 16 of the
//                 tile's rows and lx, lx + 16 of its columns.  The planes of
//                 the 64 samples go through LDS in chunks of
//                 VCFC_KIN_CHUNK_WORDS variant words, at an odd pitch: the
//                 lanes of a wave read 16 consecutive column samples (different
//                 banks) and 4 row samples (one address each).  Nine AND +
//                 population counts per pair and word, the other five cells by
//                 subtraction, as k_ld_pairs.  The tables leave through LDS:
//                 runs of 16 tables (144 dwords) of a row of the square, and
//                 for a tile off the diagonal the transposed tables as runs of
//                 row j.  Every cell has one owner: accumulate is a plain
//                 load-add-store.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <vcfc_wave.h>   // angle brackets: tests/simt_emu shadows it
#include "vcfc_bed_planes.h"
#include "vcfc_device.h"

namespace {

constexpr uint32_t KIN_T = VCFC_KIN_TILE_SAMPLES;
constexpr uint32_t KIN_CH = VCFC_KIN_CHUNK_WORDS;
constexpr uint32_t KIN_PITCH = 3 * KIN_CH + 1;            // odd: consecutive samples on different banks
constexpr uint32_t KIN_THREADS = 256;
constexpr uint32_t KIN_H = KIN_T / 2;                     // a lane's two samples are KIN_H apart
constexpr uint32_t KIN_OPITCH = KIN_H * 9 + 1;            // a row of 16 tables in the output staging; odd
constexpr uint32_t KIN_PR = VCFC_KIN_PLANE_ROWS;
constexpr uint32_t KIN_PW = KIN_PR / 32;                  // plane words of a sample a block of k_kin_planes writes
constexpr uint32_t KIN_PS = 4;                            // sample words (of 32 samples) a block of k_kin_planes covers
static_assert(KIN_CH % 4 == 0 && KIN_T == 32 && KIN_H * KIN_H == KIN_THREADS, "16-byte staging; 2 x 2 pairs a lane");
static_assert(KIN_PR == KIN_THREADS && KIN_PR % 64 == 0, "a lane a row; a wave 64 rows");

__global__ void k_kin_reset(VcfcKinArgs a) {
    if (threadIdx.x != 0) return;
    uint64_t rows = a.n;
    if (a.row_of) {
        rows = a.row_of[a.n];
        const uint64_t e = *a.err;
        if ((e & 0xFFull) == 3ull && (e >> 8) < a.n) rows = a.row_of[e >> 8];
    }
    a.state[0] = std::min<uint64_t>(rows, a.n);
    if (a.own_err) *a.err = ~0ull;
}

__global__ __launch_bounds__(KIN_THREADS) void k_kin_planes(VcfcKinArgs a) {
    __shared__ uint32_t t[3 * 32 * KIN_PW];
    const uint64_t rows = a.state[0], RW = a.row_words;
    const uint32_t S = (uint32_t)a.S, rb = (S + 3u) >> 2, nw = (S + 31u) >> 5;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t nsg = (nw + KIN_PS - 1) / KIN_PS, tiles = nsg * ((RW + KIN_PW - 1) / KIN_PW);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t rg = tile / nsg;
        const uint32_t sg = (uint32_t)(tile % nsg);
        const uint64_t r = rg * KIN_PR + tid;
        for (uint32_t k = 0; k < KIN_PS; k++) {
            const uint32_t w = sg * KIN_PS + k;
            if (w >= nw) break;   // (the whole block)
            uint32_t H = 0, B = 0, V = 0;
            if (r < rows) vcfc_bed::word_planes(a.bed + r * a.row_stride + 8ull * w, w, S, rb, H, B, V);
            uint64_t mh = 0, mb = 0, mv = 0;   // lane b < 32: sample 32 w + b's 64 rows
#pragma unroll
            for (uint32_t b = 0; b < 32; b++) {
                const uint64_t h = vw::ballot((H >> b) & 1u), g = vw::ballot((B >> b) & 1u), v = vw::ballot((V >> b) & 1u);
                if (lane == b) {
                    mh = h;
                    mb = g;
                    mv = v;
                }
            }
            __syncthreads();   // the previous sample word has left t
            if (lane < 32) {
                uint32_t *o = t + lane * KIN_PW + 2u * wave;
                o[0] = (uint32_t)mh;
                o[1] = (uint32_t)(mh >> 32);
                o[32 * KIN_PW] = (uint32_t)mb;
                o[32 * KIN_PW + 1] = (uint32_t)(mb >> 32);
                o[64 * KIN_PW] = (uint32_t)mv;
                o[64 * KIN_PW + 1] = (uint32_t)(mv >> 32);
            }
            __syncthreads();
            for (uint32_t e = tid; e < 3u * 32u * KIN_PW; e += KIN_THREADS) {
                const uint32_t p = e / (32u * KIN_PW), b = e / KIN_PW % 32u, x = e % KIN_PW;
                const uint64_t s = 32ull * w + b, word = rg * KIN_PW + x;
                if (s < S && word < RW) a.planes[(3ull * s + p) * RW + word] = t[e];
            }
        }
    }
}

// samples [s0, s0 + 32), words [c0, c0 + KIN_CH) of the planes into t (sample
// pitch KIN_PITCH, the three planes KIN_CH apart); a sample >= S and a word >=
// row_words as 0
__device__ __forceinline__ void kin_stage(const VcfcKinArgs &a, uint32_t *t, uint64_t s0, uint64_t c0) {
    const uint64_t RW = a.row_words;
    for (uint32_t e = threadIdx.x; e < KIN_T * 3u * (KIN_CH / 4u); e += KIN_THREADS) {
        const uint32_t sl = e / (3u * (KIN_CH / 4u)), rem = e % (3u * (KIN_CH / 4u));
        const uint32_t pl = rem / (KIN_CH / 4u), w = 4u * (rem % (KIN_CH / 4u));
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (s0 + sl < a.S && c0 + w < RW) v = *reinterpret_cast<const uint4 *>(a.planes + (3ull * (s0 + sl) + pl) * RW + c0 + w);
        uint32_t *d = t + sl * KIN_PITCH + pl * KIN_CH + w;
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
}

__device__ __forceinline__ void kin_put(uint32_t *o, uint32_t v, int accumulate) { *o = accumulate ? *o + v : v; }

__global__ __launch_bounds__(KIN_THREADS) void k_kin_pairs(VcfcKinArgs a) {
    __shared__ uint32_t st[2 * KIN_T * KIN_PITCH];   // the tile's row samples, then its column samples
    __shared__ uint32_t ot[KIN_H * KIN_OPITCH];
    const uint64_t S = a.S, T = (S + KIN_T - 1) / KIN_T, tiles = T * (T + 1) / 2;
    const uint64_t nwords = (a.state[0] + 31) / 32;
    const uint32_t tid = threadIdx.x, ly = tid / KIN_H, lx = tid % KIN_H;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        // tile = ti * T - ti (ti - 1) / 2 + tj - ti, ti <= tj < T
        const double b2 = (double)(2 * T + 1);
        const double rad = b2 * b2 - 8.0 * (double)tile;   // > 0 in exact arithmetic; clamped against rounding at T near 2^25
        uint64_t ti = (uint64_t)((b2 - sqrt(rad > 0.0 ? rad : 0.0)) * 0.5);
        if (ti >= T) ti = T - 1;
        while (ti * T - ti * (ti - 1) / 2 > tile) ti--;
        while (ti + 1 < T && (ti + 1) * T - (ti + 1) * ti / 2 <= tile) ti++;
        const uint64_t tj = ti + (tile - (ti * T - ti * (ti - 1) / 2));
        const uint64_t i0 = ti * KIN_T, j0 = tj * KIN_T;
        uint32_t acc[2][2][9];
#pragma unroll
        for (uint32_t p = 0; p < 4; p++)
#pragma unroll
            for (uint32_t e = 0; e < 9; e++) acc[p >> 1][p & 1][e] = 0;
        for (uint64_t c0 = 0; c0 < nwords; c0 += KIN_CH) {
            __syncthreads();   // the previous chunk has been read
            kin_stage(a, st, i0, c0);
            kin_stage(a, st + KIN_T * KIN_PITCH, j0, c0);
            __syncthreads();
            const uint32_t cw = (uint32_t)std::min<uint64_t>(KIN_CH, nwords - c0);
            const uint32_t *x = st + ly * KIN_PITCH, *y = st + (KIN_T + lx) * KIN_PITCH;
            for (uint32_t w = 0; w < cw; w++) {
                uint32_t hi[2], bi[2], vi[2], hj[2], bj[2], vj[2];
#pragma unroll
                for (uint32_t q = 0; q < 2; q++) {
                    hi[q] = x[q * KIN_H * KIN_PITCH + w];
                    bi[q] = x[q * KIN_H * KIN_PITCH + KIN_CH + w];
                    vi[q] = x[q * KIN_H * KIN_PITCH + 2 * KIN_CH + w];
                    hj[q] = y[q * KIN_H * KIN_PITCH + w];
                    bj[q] = y[q * KIN_H * KIN_PITCH + KIN_CH + w];
                    vj[q] = y[q * KIN_H * KIN_PITCH + 2 * KIN_CH + w];
                }
#pragma unroll
                for (uint32_t p = 0; p < 2; p++)
#pragma unroll
                    for (uint32_t q = 0; q < 2; q++) {
                        uint32_t *c = acc[p][q];
                        c[0] += __builtin_popcount(hi[p] & hj[q]);
                        c[1] += __builtin_popcount(hi[p] & bj[q]);
                        c[2] += __builtin_popcount(bi[p] & hj[q]);
                        c[3] += __builtin_popcount(bi[p] & bj[q]);
                        c[4] += __builtin_popcount(hi[p] & vj[q]);
                        c[5] += __builtin_popcount(bi[p] & vj[q]);
                        c[6] += __builtin_popcount(vi[p] & hj[q]);
                        c[7] += __builtin_popcount(vi[p] & bj[q]);
                        c[8] += __builtin_popcount(vi[p] & vj[q]);
                    }
            }
        }
        // a pass: the 16 x 16 tables of samples (i0 + 16 p + ly, j0 + 16 q + lx) through LDS
#pragma unroll
        for (uint32_t p = 0; p < 2; p++)
#pragma unroll
            for (uint32_t q = 0; q < 2; q++) {
                const uint32_t *c = acc[p][q];
                const uint32_t n11 = c[0], n12 = c[1], n21 = c[2], n22 = c[3];
                const uint32_t r1 = c[4], r2 = c[5], c1 = c[6], c2 = c[7], N = c[8];
                __syncthreads();   // the previous pass has left ot
                uint32_t *o = ot + ly * KIN_OPITCH + lx * 9u;
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
                const uint64_t ib = i0 + KIN_H * p, jb = j0 + KIN_H * q;
                for (uint32_t d = tid; d < KIN_H * KIN_H * 9u; d += KIN_THREADS) {
                    const uint32_t il = d / (KIN_H * 9u), rem = d % (KIN_H * 9u);
                    if (ib + il < S && jb + rem / 9u < S)
                        kin_put(a.tables + ((ib + il) * S + jb) * 9ull + rem, ot[il * KIN_OPITCH + rem], a.accumulate);
                }
                if (ti == tj) continue;   // (the whole block) the diagonal tile computed both orders
                for (uint32_t d = tid; d < KIN_H * KIN_H * 9u; d += KIN_THREADS) {
                    const uint32_t jl = d / (KIN_H * 9u), rem = d % (KIN_H * 9u), il = rem / 9u, e = rem % 9u;
                    if (ib + il < S && jb + jl < S)
                        kin_put(a.tables + ((jb + jl) * S + ib) * 9ull + rem, ot[il * KIN_OPITCH + jl * 9u + (e % 3u) * 3u + e / 3u],
                                a.accumulate);
                }
            }
    }
}

}  // namespace

VcfcKinLayout vcfc_kin_workspace_layout(uint64_t n, uint64_t S) {
    auto al = [](uint64_t x) { return (x + 255) & ~255ull; };
    VcfcKinLayout L;
    L.row_words = (((n + 31) / 32) + 3) & ~3ull;
    L.bed_stride = (vcfc_matrix_row_size(VCFC_MATRIX_BED, S) + 15) & ~15ull;
    uint64_t o = 0;
    L.state = o; o = al(o + 16);
    L.planes = o; o = al(o + 12 * L.row_words * S);
    L.bed = o; o = al(o + L.bed_stride * n + 64);
    L.matrix = o; o = al(o + vcfc_matrix_workspace_layout(n).total);
    L.total = o;
    return L;
}

hipError_t vcfc_kin_run(const VcfcKinArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_kin_reset, dim3(1), dim3(64), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.n) {
        const uint64_t want = ((a.S + 32 * KIN_PS - 1) / (32 * KIN_PS)) * ((a.row_words + KIN_PW - 1) / KIN_PW);
        hipLaunchKernelGGL(k_kin_planes, dim3((unsigned)std::min<uint64_t>(want, 1u << 20)), dim3(KIN_THREADS), 0, s, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const uint64_t T = (a.S + KIN_T - 1) / KIN_T;
    hipLaunchKernelGGL(k_kin_pairs, dim3((unsigned)std::min<uint64_t>(T * (T + 1) / 2, 1u << 22)), dim3(KIN_THREADS), 0, s, a);
    return hipGetLastError();
}
