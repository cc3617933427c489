// vcfc_matrix.hip -- gfx950 kernels of genotype-matrix: per
// (selected) record one row of the variants x samples matrix, written out of
// the run-length code: a run byte is a class and a count, and the row is that
// class's value written `count` times at the run's place in the prefix sum
// over item counts.  Three layouts: int8 dosage (S bytes), the two int8
// haplotype planes interleaved (2 S bytes), PLINK 1 .bed codes (2 bits a
// sample, ceil(S / 4) bytes).
//
//   k_gm_reset    the call's state (err, the queue's count; row_of[0] of an
//                 empty call), so the call can be captured and replayed.
//   k_gm_iota /   row_of[i] = i without a select array; with one, its flags as
//   k_gm_flags    words, then the project's u32 -> u64 exclusive scan.
//   k_gm_scan     a resident grid (S <= vcfc_matrix_tile_samples); a wave owns
//                 an LDS row tile and takes chunks of 16 consecutive records,
//                 dealt round-robin over the grid.  One wave per record: the
//                 frame is checked (frame_open), the tile is filled with the
//                 0|0 value, the sample section is scanned in 256-byte windows
//                 (scan_window) and every item start that is not a 0|0 run
//                 writes its columns into the tile.  A window's items are
//                 written only after the running token count with the whole
//                 window included has been checked against S, so no column
//                 >= S is ever touched.  The tile sits in LDS at the row's
//                 address modulo 16 and goes out once: a byte head, 16-byte
//                 stores, a byte tail, nothing outside [row, row + row_bytes).
//                 .bed: the tile holds one code byte per sample and is packed
//                 (one v_dot4_u32_u8 per output byte) before the store.  A
//                 record that is not simple (the decoder's sense) writes
//                 nothing and is queued.
//   k_gm_seq      one lane per queued record (or, above the tile limit, per
//                 selected record): the byte-serial walk of a regular record
//                 (walk_regular) writes the same bytes straight to the row,
//                 or reports error code 3.
//
// A row that would end past out_cap is reported (code 0xFF) before the record
// is read, and not written.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vcfc_wave.h>   // angle brackets: tests/simt_emu shadows it
#include "vcfc_device.h"
#include "vcfc_decode_dev.h"

namespace {

constexpr int GM_WAVES = 4;           // waves per block
constexpr uint32_t GM_CH = 16;        // consecutive records a wave takes at a time
constexpr uint32_t GM_TILE = VCFC_MATRIX_TILE_BYTES;
constexpr uint32_t GM_BED_CODES = 4096;   // .bed: code bytes [0, 4096), the packed row behind them
constexpr int GM_BLOCKS_PER_CU = 5;   // what 4 x (SBUF + GM_TILE) bytes of LDS leave resident

// The four values of a token: GT ends at the first ':',
// pieces split at '|' and '/', a piece of digits is called with class
// min(2, value), every other piece is missing.  at(k): byte k of the token.
struct Codes {
    uint32_t dos, h0, h1, bed;   // (int8 values as their low byte)
};
template <class F>
__device__ __forceinline__ Codes tok_codes(F at, uint32_t len) {
    uint32_t v = 0, piece = 0, nz = 0, h0 = 0xFFu, h1 = 0xFFu;
    bool digits = false, other = false, missing = false;
    for (uint32_t k = 0;; k++) {
        const uint32_t b = k < len ? at(k) : ':';
        if (b == ':' || b == '|' || b == '/') {
            if (digits && !other) {
                if (piece == 0) h0 = v;
                else if (piece == 1) h1 = v;
                nz += v != 0;
            } else {
                missing = true;
            }
            piece++;
            v = 0;
            digits = other = false;
            if (b == ':') break;
        } else if (b >= '0' && b <= '9') {
            digits = true;
            v = umin32(2u, 10u * v + (b - '0'));
        } else {
            other = true;
        }
    }
    Codes c;
    c.dos = missing ? 0xFFu : umin32(nz, 127u);
    c.h0 = h0;
    c.h1 = h1;
    c.bed = piece == 2 && !missing && h0 < 2u && h1 < 2u ? (h0 + h1 == 0 ? 3u : h0 + h1 == 1 ? 2u : 0u) : 1u;
    return c;
}

// a class run's byte (>= 0x80, not an escape): 0|1 -> 0xA0, 1|0 -> 0xC0, 1|1 -> 0x80
__device__ __forceinline__ Codes run_codes(uint32_t b) {
    const uint32_t m = b & 0xE0u;
    Codes c;
    c.h0 = m == 0xA0u ? 0u : 1u;
    c.h1 = m == 0xC0u ? 0u : 1u;
    c.dos = c.h0 + c.h1;
    c.bed = c.dos == 2u ? 0u : 2u;
    return c;
}

// column col of a tile (volatile: two adjacent byte stores stay two, the
// pair may lie at an odd address)
template <int LAYOUT>
__device__ __forceinline__ void tile_put(volatile uint8_t *t, uint32_t col, const Codes &c) {
    if (LAYOUT == VCFC_MATRIX_DOSAGE) {
        t[col] = (uint8_t)c.dos;
    } else if (LAYOUT == VCFC_MATRIX_HAP) {
        t[2 * col] = (uint8_t)c.h0;
        t[2 * col + 1] = (uint8_t)c.h1;
    } else {
        t[col] = (uint8_t)c.bed;
    }
}

// whether row r of rb bytes ends inside out_cap (no product overflows)
__device__ __forceinline__ bool row_fits(const VcfcMatrixArgs &a, uint64_t r, uint64_t rb) {
    return r <= a.out_cap / a.row_stride && a.out_cap - r * a.row_stride >= rb;
}

// t[al, al + nb) -> row[0, nb), t 16-byte aligned and al = row's address
// modulo 16: a byte head up to the first 16-byte boundary, 16-byte stores, a
// byte tail; no byte outside the row is written
__device__ __forceinline__ void store_row(const uint8_t *t, uint32_t al, uint8_t *row, uint32_t nb) {
    const uint32_t l = vw::lane_id();
    const uint32_t head = umin32(nb, (16u - al) & 15u);
    if (l < head) row[l] = t[al + l];
    const uint32_t body = (nb - head) >> 4;
    // non-temporal: no kernel of the call reads a row back (hap -7.5 %, dosage -1.5 % against plain
    // stores, profiles/matrix/ab/nt_store_*)
    for (uint32_t k = l; k < body; k += 64)
        vw::gstore16_nt(row, head + 16ull * k, *reinterpret_cast<const uint4 *>(t + al + head + 16u * k));
    const uint32_t tail = head + 16u * body;
    if (tail + l < nb) row[tail + l] = t[al + tail + l];
}

// One record, one wave.  false: not simple, nothing of it is written (the
// caller queues it).
template <int LAYOUT>
__device__ __forceinline__ bool expand_one(const VcfcMatrixArgs &a, uint64_t i, uint8_t *sb, uint8_t *tile) {
    const uint32_t l = vw::lane_id();
    const uint32_t S = (uint32_t)a.S;
    const uint32_t rb = (uint32_t)vcfc_matrix_row_size(LAYOUT, S);
    const uint64_t r = a.row_of[i];
    if (!row_fits(a, r, rb)) {
        if (l == 0) atomicMin((unsigned long long *)a.err, (unsigned long long)((i << 8) | 0xFFu));
        return true;
    }
    uint8_t *row = a.out + r * a.row_stride;
    const uint32_t al = (uint32_t)(reinterpret_cast<uintptr_t>(row) & 15u);
    RecFrame f;
    if (!frame_open(f, sb, a.in, a.rec_start[i], a.rec_start[i + 1]) || f.slen != f.req) return false;   // (no NUL in REQ)
    Staged &sg = f.sg;
    const uint32_t s0 = f.s0(), s1 = f.s1();
    // the tile as a row of 0|0: 0, (0, 0) or code 3; .bed's pad samples are code 0
    vw::wave_sync();   // the previous record's store has read the tile
    {
        const uint32_t n16 = LAYOUT == VCFC_MATRIX_BED ? (S + 15u) >> 4 : (al + rb + 15u) >> 4;
        const uint32_t w = LAYOUT == VCFC_MATRIX_BED ? 0x03030303u : 0u;
        for (uint32_t k = l; k < n16; k += 64) reinterpret_cast<uint4 *>(tile)[k] = make_uint4(w, w, w, w);
        vw::wave_sync();
        if (LAYOUT == VCFC_MATRIX_BED && l < ((4u - (S & 3u)) & 3u)) tile[S + l] = 0;
        vw::wave_sync();
    }
    uint8_t *t = LAYOUT == VCFC_MATRIX_BED ? tile : tile + al;
    ItemState st;
    for (uint32_t cur = s0 & ~3u; cur < s1; cur += 256) {
        sg.need(cur, 256 + 8);
        const uint32_t b = umin32(cur + 256, s1);
        const uint32_t v4 = sg.at4(cur + 4 * l);
        const ItemLane it = scan_window(v4, cur, s0, b, s1, st);
        // checked before any item of the window is written: every column below is < st.got <= S
        if (st.bad || st.got > S) return false;
        const uint32_t hi = msb4(v4) & it.start;   // class runs and escapes
        if (vw::ballot(hi != 0) == 0) continue;    // a window of 0|0 runs
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            if (!((hi >> j) & 1u)) continue;
            const uint32_t bt = (v4 >> (8 * j)) & 0xFFu;
            if ((bt & 0xE0u) == 0xE0u) {   // (simple: 0xE1, 3 payload bytes and a TAB, inside the record)
                const uint32_t p = cur + 4 * l + j;
                const uint32_t w = sg.at(p + 1) | (sg.at(p + 2) << 8) | (sg.at(p + 3) << 16);
                tile_put<LAYOUT>(t, it.gb[j], tok_codes([&](uint32_t q) { return (w >> (8 * q)) & 0xFFu; }, 3u));
            } else {
                const Codes c = run_codes(bt);
                const uint32_t cnt = bt & 0x1Fu;
                for (uint32_t k = 0; k < cnt; k++) tile_put<LAYOUT>(t, it.gb[j] + k, c);
            }
        }
    }
    if (st.got != S) return false;
    vw::wave_sync();
    if (LAYOUT == VCFC_MATRIX_BED) {
        uint8_t *packed = tile + GM_BED_CODES;
        for (uint32_t k = l; k < rb; k += 64)
            packed[al + k] = (uint8_t)vw::dot4u(reinterpret_cast<const uint32_t *>(tile)[k], 0x40100401u, 0u);
        vw::wave_sync();
        store_row(packed, al, row, rb);
    } else {
        store_row(tile, al, row, rb);
    }
    return true;
}

template <bool SEL, int LAYOUT>
__global__ __launch_bounds__(64 * GM_WAVES) void k_gm_scan(VcfcMatrixArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t sbuf[GM_WAVES * SBUF];
    __shared__ __attribute__((aligned(16))) uint8_t tiles[GM_WAVES * GM_TILE];
    const uint32_t wave = vw::readfirst(threadIdx.x >> 6);
    const uint32_t l = vw::lane_id();
    uint8_t *sb = sbuf + wave * SBUF;
    uint8_t *tile = tiles + wave * GM_TILE;
    // chunks of GM_CH consecutive records, dealt round-robin to the grid's
    // waves: the records a query selects are neighbours, and spread over all blocks
    const uint64_t stride = (uint64_t)gridDim.x * GM_WAVES * GM_CH;
    for (uint64_t c0 = ((uint64_t)blockIdx.x * GM_WAVES + wave) * GM_CH; c0 < a.n; c0 += stride) {
        const uint64_t il = c0 + l;
        const bool on = l < GM_CH && il < a.n && (!SEL || a.select[il]);
        for (uint64_t m = vw::ballot(on); m; m &= m - 1) {
            const uint64_t i = c0 + (uint64_t)__builtin_ctzll(m);
            if (!expand_one<LAYOUT>(a, i, sb, tile) && l == 0) {
                const uint32_t q = atomicAdd(a.seq_count, 1u);
                a.seq_list[q] = (uint32_t)i;
            }
        }
    }
}

// The byte-serial walk of a regular record (walk_regular, vcfc_decode_dev.h),
// one lane: its row straight to global memory; false where the record is not
// regular (its row is not meaningful then).  Every column written is below S:
// walk_regular checks an item's count against S before it reports the item.
template <int LAYOUT>
__device__ bool gm_walk(const VcfcMatrixArgs &a, uint64_t i) {
    const uint64_t rb = vcfc_matrix_row_size(LAYOUT, a.S);
    const uint64_t r = a.row_of[i];
    if (!row_fits(a, r, rb)) {
        atomicMin((unsigned long long *)a.err, (unsigned long long)((i << 8) | 0xFFu));
        return true;
    }
    uint8_t *row = a.out + r * a.row_stride;
    uint32_t acc = 0;   // .bed: the codes of the byte being filled (columns come in order)
    auto put = [&](uint64_t col, const Codes &c) {
        if (LAYOUT == VCFC_MATRIX_DOSAGE) {
            row[col] = (uint8_t)c.dos;
        } else if (LAYOUT == VCFC_MATRIX_HAP) {
            row[2 * col] = (uint8_t)c.h0;
            row[2 * col + 1] = (uint8_t)c.h1;
        } else {
            acc |= c.bed << (2u * ((uint32_t)col & 3u));
            if ((col & 3u) == 3u) {
                row[col >> 2] = (uint8_t)acc;
                acc = 0;
            }
        }
    };
    const bool ok = walk_regular<true>(
        a.in, a.rec_start[i], a.rec_start[i + 1], a.S,
        [&](uint64_t got, const uint8_t *src, uint32_t len) {
            put(got, tok_codes([&](uint32_t q) { return (uint32_t)src[q]; }, len));
        },
        [&](uint8_t b, uint64_t got, uint32_t cnt) {
            Codes c;
            if (b < 0x80u) {   // a 0|0 run
                c.dos = c.h0 = c.h1 = 0u;
                c.bed = 3u;
            } else {
                c = run_codes(b);
            }
            for (uint32_t k = 0; k < cnt; k++) put(got + k, c);
        });
    if (!ok) return false;
    if (LAYOUT == VCFC_MATRIX_BED && (a.S & 3u)) row[a.S >> 2] = (uint8_t)acc;   // the pad bits are 0
    return true;
}

// ALL: every (selected) record, one lane each; else the queued ones.
template <int LAYOUT, bool ALL>
__global__ __launch_bounds__(256) void k_gm_seq(VcfcMatrixArgs a) {
    const uint64_t cnt = ALL ? a.n : *a.seq_count;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < cnt; q += (uint64_t)gridDim.x * blockDim.x) {
        if (ALL && a.select && !a.select[q]) continue;
        const uint64_t i = ALL ? q : a.seq_list[q];
        if (!gm_walk<LAYOUT>(a, i)) atomicMin((unsigned long long *)a.err, (unsigned long long)((i << 8) | 3u));
    }
}

__global__ void k_gm_reset(uint64_t *err, uint32_t *seq_count, uint64_t *row_of, uint64_t n) {
    if (threadIdx.x == 0) {
        *err = ~0ull;
        *seq_count = 0;
        if (n == 0) row_of[0] = 0;
    }
}

__global__ __launch_bounds__(256) void k_gm_iota(uint64_t *row_of, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) row_of[i] = i;
}

__global__ __launch_bounds__(256) void k_gm_flags(const uint8_t *select, uint32_t *flag32, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag32[i] = select[i] != 0;
}

// as many blocks of k_gm_scan as stay resident on the current device, so a
// wave's tile and staging buffer serve many records
hipError_t resident_blocks(uint64_t *blocks) {
    int dev = 0, cus = 0;
    hipError_t e;
    if ((e = hipGetDevice(&dev)) != hipSuccess ||
        (e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess)
        return e;
    *blocks = (uint64_t)GM_BLOCKS_PER_CU * (uint64_t)(cus > 0 ? cus : 1);
    return hipSuccess;
}

template <int LAYOUT>
hipError_t launch_rows(const VcfcMatrixArgs &a, hipStream_t s) {
    const uint64_t want = (a.n + 255) / 256;
    const dim3 sg((unsigned)(want < 1024 ? want : 1024));
    if (a.S > vcfc_matrix_tile_samples(LAYOUT)) {
        hipLaunchKernelGGL((k_gm_seq<LAYOUT, true>), sg, dim3(256), 0, s, a);
        return hipGetLastError();
    }
    const uint64_t chunk = (uint64_t)GM_WAVES * GM_CH;
    uint64_t max_blocks = 0;
    hipError_t e = resident_blocks(&max_blocks);
    if (e != hipSuccess) return e;
    const unsigned g = (unsigned)std::min<uint64_t>(max_blocks, (a.n + chunk - 1) / chunk);
    if (a.select) hipLaunchKernelGGL((k_gm_scan<true, LAYOUT>), dim3(g), dim3(64 * GM_WAVES), 0, s, a);
    else hipLaunchKernelGGL((k_gm_scan<false, LAYOUT>), dim3(g), dim3(64 * GM_WAVES), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((k_gm_seq<LAYOUT, false>), sg, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace

uint64_t vcfc_matrix_scan_trip(int layout) {
    uint64_t blocks = 0;
    if (vcfc_matrix_tile_samples(layout) == 0 || resident_blocks(&blocks) != hipSuccess) return 0;
    return blocks * GM_WAVES * GM_CH;
}

VcfcMatrixLayout vcfc_matrix_workspace_layout(uint64_t n) {
    auto al = [](uint64_t x) { return (x + 255) & ~255ull; };
    VcfcMatrixLayout L;
    uint64_t o = 0;
    L.flag32 = o; o = al(o + 4 * (n + 1));
    L.partials = o; o = al(o + 8 * ((n + 4095) / 4096 + 1));
    L.seq_list = o; o = al(o + 4 * (n + 1));
    L.seq_count = o; o = al(o + 8);
    L.total = o;
    return L;
}

hipError_t vcfc_matrix_run(const VcfcMatrixArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_gm_reset, dim3(1), dim3(64), 0, s, a.err, a.seq_count, a.row_of, a.n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.n == 0) return e;
    if (a.select) {
        hipLaunchKernelGGL(k_gm_flags, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a.select, a.flag32, a.n);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = vcfc_scan_u32(a.flag32, a.n, a.partials, a.row_of, s)) != hipSuccess) return e;
    } else {
        hipLaunchKernelGGL(k_gm_iota, dim3((unsigned)(a.n / 256 + 1)), dim3(256), 0, s, a.row_of, a.n);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    switch (a.layout) {
    case VCFC_MATRIX_DOSAGE: return launch_rows<VCFC_MATRIX_DOSAGE>(a, s);
    case VCFC_MATRIX_HAP: return launch_rows<VCFC_MATRIX_HAP>(a, s);
    default: return launch_rows<VCFC_MATRIX_BED>(a, s);
    }
}
