// vcfc_subset.hip -- gfx950 kernels of the sample-subset decoder (DESIGN.md
// §4i): REQ and K chosen sample columns of every record, found in the
// compressed domain.  The run-length code makes a sample's token a prefix-sum
// lookup over run counts, so the work follows the record bytes and K, not S.
//
//   k_sub_plan   one wave per record: is the record "simple" (the decoder's
//                sense, vcfc_decode.hip) and its REQ free of NULs?  Then its
//                line is REQ + 4 K bytes.  Others are queued.
//   k_sub_seq    one lane per queued record: the byte-serial walk of a
//                regular record (size, or error code 3).
//   scan         line offsets (the encoder's exclusive scan).
//   k_sub_write  one wave per record, simple records: the sample section is
//                scanned in 256-byte windows (scan_window, shared with the
//                decoder); the wave keeps a cursor into the ascending column
//                list, takes the columns that fall inside a window 64 at a
//                time, finds each one's item by a binary search over the
//                window's per-byte token prefix values in LDS, and puts its
//                word "a|b\t" at slot `rank` of the line's sample part, which
//                is assembled in LDS and leaves as contiguous 16-byte stores
//                (K <= SUB_TK; above that the words go straight to memory).
//   k_sub_wseq   a fixed number of lanes over the queue: the byte-serial
//                writer (token lengths by rank, prefix sum, copy).
//
// The plan is exact (every record is read twice), so one call gives exact
// line offsets with no host round trip: DESIGN.md §4i says why.
#include <hip/hip_runtime.h>
#include <vcfc_wave.h>   // angle brackets: tests/simt_emu shadows it
#include "vcfc_device.h"
#include "vcfc_decode_dev.h"

namespace {

constexpr int SUB_WAVES = 4;          // records per 256-thread block
constexpr uint32_t SUB_TK = 512;      // words of the LDS line tile per wave

constexpr uint32_t SS_SIMPLE = 0;     // line = REQ + 4K bytes, wave-parallel
constexpr uint32_t SS_SEQ = 1;        // regular, byte-serial
constexpr uint32_t SS_ERR = 3;        // not regular
constexpr uint32_t SS_SKIP = 5;       // not selected: no line

constexpr int SW_SIZE = 0, SW_LEN = 1, SW_WRITE = 2;

// The byte-serial walk of a regular record (walk_regular, vcfc_decode_dev.h)
// [rs, re): false where the record is not regular.  SW_SIZE: checks
// everything, *size = the line's bytes.  SW_LEN: scr[rank] = length of each
// chosen token.  SW_WRITE: the chosen tokens and their TAB / LF to tok +
// scr[rank] (scr: offsets).
template <int MODE>
__device__ bool sub_walk(const VcfcSubsetArgs &a, uint64_t rs, uint64_t re, uint32_t *scr, uint8_t *tok,
                         uint64_t *size) {
    uint64_t sum = 0;
    uint32_t c = 0;
    const uint32_t K = a.K;
    auto emit = [&](const uint8_t *src, uint32_t len) {   // the token of column csort[c]
        const uint32_t r = a.rank[c];
        if (MODE == SW_SIZE) sum += len;
        else if (MODE == SW_LEN) scr[r] = len;
        else {
            uint8_t *o = tok + scr[r];
            for (uint32_t k = 0; k < len; k++) o[k] = src[k];
            o[len] = r + 1 == K ? '\n' : '\t';
        }
        c++;
    };
    const bool ok = walk_regular<MODE == SW_SIZE>(
        a.in, rs, re, a.S,
        [&](uint64_t got, const uint8_t *src, uint32_t len) {
            if (c < K && a.csort[c] == got) emit(src, len);
        },
        [&](uint8_t b, uint64_t got, uint32_t cnt) {
            const uint32_t m = b & 0xE0u;   // 0|1 -> 0xA0, 1|0 -> 0xC0, 1|1 -> 0x80, 0|0 < 0x80
            const uint8_t w[3] = {(uint8_t)(b < 0x80u || m == 0xA0u ? '0' : '1'), '|',
                                  (uint8_t)(b < 0x80u || m == 0xC0u ? '0' : '1')};
            while (c < K && a.csort[c] < got + cnt) emit(w, 3);
        });
    if (ok && MODE == SW_SIZE) *size = (uint64_t)be30(a.in + rs + 4) + sum + K;
    return ok;
}

// One record, one wave: simple (line size req + 4K) or queued.
__device__ __forceinline__ void plan_one(const VcfcSubsetArgs &a, uint64_t i, uint8_t *sb) {
    const uint32_t l = vw::lane_id();
    const uint64_t rs_abs = a.rec_start[i], re_abs = a.rec_start[i + 1];
    bool simple = false;
    uint64_t size = 0;
    RecFrame f;
    if (frame_open(f, sb, a.in, rs_abs, re_abs) && f.slen == f.req) {   // (no NUL in REQ)
        const ItemState st = scan_items_plain(f);
        size = (uint64_t)f.req + 4ull * a.K;
        simple = !st.bad && st.got == a.S && size <= 0xFFFFFFFFull;
    }
    if (l == 0) {
        a.st[i] = simple ? SS_SIMPLE : SS_SEQ;
        a.line_size[i] = simple ? (uint32_t)size : 0u;
        if (!simple) {
            const uint32_t q = atomicAdd(a.seq_count, 1u);
            a.seq_list[q] = (uint32_t)i;
        }
    }
}

// (selected mode, a.select set: the dealing of SEL_R records to a wave,
// vcfc_decode_dev.h)
template <bool SEL>
__global__ __launch_bounds__(256) void k_sub_plan(VcfcSubsetArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t sbuf[SUB_WAVES * SBUF];
    const uint32_t wave = vw::readfirst(threadIdx.x >> 6);
    uint8_t *sb = sbuf + wave * SBUF;
    const uint64_t g = (uint64_t)blockIdx.x * SUB_WAVES + wave;
    if (!SEL) {
        if (g < a.n) plan_one(a, g, sb);
        return;
    }
    const uint64_t G = (uint64_t)gridDim.x * SUB_WAVES;
    const uint32_t l = vw::lane_id();
    const uint64_t il = g + (uint64_t)l * G;
    const bool mine = l < SEL_R && il < a.n;
    const bool on = mine && a.select[il];
    if (mine && !on) { a.st[il] = SS_SKIP; a.line_size[il] = 0; }
    for (uint64_t m = vw::ballot(on); m; m &= m - 1)
        plan_one(a, g + (uint64_t)__builtin_ctzll(m) * G, sb);
}

// Queued records, one lane each (grid-stride).
__global__ __launch_bounds__(256) void k_sub_seq(VcfcSubsetArgs a) {
    const uint32_t cnt = *a.seq_count;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < cnt; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = a.seq_list[q];
        uint64_t size = 0;
        const bool ok = sub_walk<SW_SIZE>(a, a.rec_start[i], a.rec_start[i + 1], nullptr, nullptr, &size) &&
                        size <= 0xFFFFFFFFull;
        a.st[i] = ok ? SS_SEQ : SS_ERR;
        a.line_size[i] = ok ? (uint32_t)size : 0u;
        if (!ok) atomicMin((unsigned long long *)a.err, (unsigned long long)((i << 8) | 3u));
    }
}

// The line of simple record i: REQ, then the chosen tokens' words.  G: 256
// words (the window's per-byte token prefix), W: SUB_TK words (the line's
// sample part while K <= SUB_TK).
__device__ __forceinline__ void write_one(const VcfcSubsetArgs &a, uint64_t i, uint8_t *sb, uint32_t *G, uint32_t *W) {
    const uint32_t l = vw::lane_id();
    const uint32_t K = a.K;
    // everything the record's first steps need, loaded at once (one memory
    // round trip): its metadata, and the wave's next 64 chosen columns
    // (lane l: column csort[c + l] and its output slot), kept one batch ahead
    const uint64_t L0 = a.line_off[i], L1 = a.line_off[i + 1];
    const uint32_t rst = a.st[i];
    const uint64_t rs_abs = a.rec_start[i], re_abs = a.rec_start[i + 1];
    uint32_t tq = l < K ? a.csort[l] : ~0u, rq = l < K ? a.rank[l] : 0u;
    if (L1 > a.out_cap) {
        if (l == 0) atomicMin((unsigned long long *)a.err, (unsigned long long)((i << 8) | 0xFFu));
        return;
    }
    if (rst != SS_SIMPLE) return;   // queued records: k_sub_wseq; no line otherwise
    RecFrame f;
    frame_stage(f, sb, a.in, rs_abs, re_abs);
    Staged &sg = f.sg;
    const uint32_t rs = f.rs, req = f.req;
    uint8_t *line = a.out + L0;
    // REQ verbatim (4 bytes per lane, 256 per step)
    for (uint32_t b0 = 0; b0 < req; b0 += 256) {
        sg.need(rs + 8 + b0, 256);
        const uint32_t k = b0 + 4 * l;
        if (k < req) {
            uint32_t w;
            __builtin_memcpy(&w, sg.lds + (rs + 8 + k - sg.cbase), 4);   // (unaligned ds_read_b32)
            if (k + 4 <= req) {
                __builtin_memcpy(line + k, &w, 4);
            } else {
                for (uint32_t j = 0; j < 3; j++)
                    if (k + j < req) line[k + j] = (uint8_t)(w >> (8 * j));
            }
        }
    }
    uint8_t *tok = line + req;
    const bool tile = K <= SUB_TK;
    const uint32_t s0 = f.s0(), s1 = f.s1();
    ItemState st;
    uint32_t c = 0;                          // cursor into csort (wave-uniform)
    uint32_t nextt = vw::readlane(tq, 0);    // csort[c]
    for (uint32_t cur = s0 & ~3u; cur < s1 && c < K; cur += 256) {
        sg.need(cur, 256 + 8);
        const uint32_t b = umin32(cur + 256, s1);
        const ItemLane it = scan_window(sg.at4(cur + 4 * l), cur, s0, b, s1, st);
        if (nextt >= st.got) continue;   // no chosen column in this window
        // G[k] = tokens before byte k's item; it steps at item starts only,
        // so the item holding token t is the last k with G[k] <= t
        vw::wave_sync();
        *reinterpret_cast<uint4 *>(G + 4 * l) = make_uint4(it.gb[0], it.gb[1], it.gb[2], it.gb[3]);
        vw::wave_sync();
        for (;;) {
            const uint32_t t = tq;
            const bool in_win = t < st.got;   // (ascending: the lanes that hold one are the first ones)
            if (in_win) {
                uint32_t lo = 0;
#pragma unroll
                for (uint32_t step = 128; step; step >>= 1)
                    if (G[lo + step] <= t) lo += step;
                const uint32_t p = cur + lo;
                const uint32_t bt = sg.at(p);
                uint32_t w;
                if (bt == 0xE1u) {
                    w = sg.at(p + 1) | (sg.at(p + 2) << 8) | (sg.at(p + 3) << 16) | 0x09000000u;
                } else {
                    const uint32_t m = bt & 0xE0u;
                    const uint32_t x = bt < 0x80u || m == 0xA0u ? '0' : '1', y = bt < 0x80u || m == 0xC0u ? '0' : '1';
                    w = x | ((uint32_t)'|' << 8) | (y << 16) | 0x09000000u;
                }
                const uint32_t r = rq;
                if (r + 1 == K) w = (w & 0x00FFFFFFu) | 0x0A000000u;   // the line's LF
                if (tile) W[r] = w;
                else __builtin_memcpy(tok + 4ull * r, &w, 4);
            }
            const uint32_t cnt = (uint32_t)vw::popc64(vw::ballot(in_win));
            if (cnt == 0) break;
            c += cnt;
            // the next batch: in flight while the following windows are scanned
            const uint32_t q = c + l;
            tq = q < K ? a.csort[q] : ~0u;
            rq = q < K ? a.rank[q] : 0u;
            if (cnt < 64) break;
        }
        nextt = vw::readlane(tq, 0);
    }
    if (tile) {
        vw::wave_sync();
        for (uint32_t w0 = 4 * l; w0 < K; w0 += 256) {
            if (w0 + 4 <= K) {
                vw::gstore16(tok, 4ull * w0, *reinterpret_cast<const uint4 *>(W + w0));
            } else {
                for (uint32_t j = w0; j < K; j++) __builtin_memcpy(tok + 4ull * j, W + j, 4);
            }
        }
        vw::wave_sync();   // W is free for the wave's next record
    }
}

template <bool SEL>
__global__ __launch_bounds__(256) void k_sub_write(VcfcSubsetArgs a, uint64_t first, uint64_t last) {
    __shared__ __attribute__((aligned(16))) uint8_t sbuf[SUB_WAVES * SBUF];
    __shared__ __attribute__((aligned(16))) uint32_t gbuf[SUB_WAVES * 256];
    __shared__ __attribute__((aligned(16))) uint32_t tbuf[SUB_WAVES * SUB_TK];
    const uint32_t wave = vw::readfirst(threadIdx.x >> 6);
    uint8_t *sb = sbuf + wave * SBUF;
    uint32_t *G = gbuf + wave * 256;
    uint32_t *W = tbuf + wave * SUB_TK;
    const uint64_t g = (uint64_t)blockIdx.x * SUB_WAVES + wave;
    if (!SEL) {
        if (first + g < last) write_one(a, first + g, sb, G, W);
        return;
    }
    const uint64_t Gw = (uint64_t)gridDim.x * SUB_WAVES;
    const uint32_t l = vw::lane_id();
    const uint64_t il = first + g + (uint64_t)l * Gw;
    const bool cand = l < SEL_R && il < last;
    for (uint64_t m = vw::ballot(cand && a.select[il]); m; m &= m - 1)
        write_one(a, first + g + (uint64_t)__builtin_ctzll(m) * Gw, sb, G, W);
}

// The queued regular records of [first, last), one lane each, a fixed number
// of lanes (lane t owns seq_scratch[t K, (t + 1) K)): token lengths by rank,
// their prefix sum, then REQ and the tokens.
__global__ __launch_bounds__(64) void k_sub_wseq(VcfcSubsetArgs a, uint64_t first, uint64_t last) {
    const uint32_t cnt = *a.seq_count;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t *scr = a.seq_scratch + t * a.K;
    for (uint64_t q = t; q < cnt; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = a.seq_list[q];
        if (i < first || i >= last || a.st[i] != SS_SEQ) continue;
        const uint64_t L0 = a.line_off[i], L1 = a.line_off[i + 1];
        if (L1 > a.out_cap) {
            atomicMin((unsigned long long *)a.err, (unsigned long long)((i << 8) | 0xFFu));
            continue;
        }
        const uint64_t rs = a.rec_start[i], re = a.rec_start[i + 1];
        uint64_t size = 0;
        if (!sub_walk<SW_LEN>(a, rs, re, scr, nullptr, &size)) continue;   // (the plan found it regular)
        uint32_t o = 0;
        for (uint32_t r = 0; r < a.K; r++) {
            const uint32_t len = scr[r];
            scr[r] = o;
            o += len + 1;
        }
        const uint8_t *h = a.in + rs;
        const uint32_t req = be30(h + 4);
        uint8_t *line = a.out + L0;
        for (uint32_t k = 0; k < req; k++) line[k] = h[8 + k];
        (void)sub_walk<SW_WRITE>(a, rs, re, scr, line + req, &size);
    }
}

__global__ void k_sub_reset(uint64_t *err, uint32_t *seq_count, uint64_t *line_off0) {
    if (threadIdx.x == 0) {
        *err = ~0ull;
        *seq_count = 0;
        if (line_off0) *line_off0 = 0;
    }
}

}  // namespace

VcfcSubsetLayout vcfc_subset_workspace_layout(uint64_t n, uint64_t K) {
    auto al = [](uint64_t x) { return (x + 255) & ~255ull; };
    VcfcSubsetLayout L;
    uint64_t o = 0;
    L.st = o; o = al(o + 4 * (n + 1));
    L.line_size = o; o = al(o + 4 * (n + 1));
    L.seq_list = o; o = al(o + 4 * (n + 1));
    L.seq_count = o; o = al(o + 8);
    L.err = o; o = al(o + 8);
    L.partials = o; o = al(o + 8 * ((n + 4095) / 4096 + 1));
    L.csort = o; o = al(o + 4 * K);
    L.rank = o; o = al(o + 4 * K);
    L.seq_scratch = o; o = al(o + 4ull * VCFC_SUBSET_SEQ_LANES * K);
    L.total = o;
    return L;
}

hipError_t vcfc_subset_plan(const VcfcSubsetArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_sub_reset, dim3(1), dim3(64), 0, s, a.err, a.seq_count, a.n == 0 ? a.line_off : nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.n == 0) return e;
    const uint64_t per_block = SUB_WAVES * (a.select ? SEL_R : 1);
    const dim3 grid((unsigned)((a.n + per_block - 1) / per_block)), block(64 * SUB_WAVES);
    if (a.select) hipLaunchKernelGGL(k_sub_plan<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_sub_plan<false>, grid, block, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint64_t want = (a.n + 255) / 256;
    hipLaunchKernelGGL(k_sub_seq, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return vcfc_scan_u32(a.line_size, a.n, a.partials, a.line_off, s);
}

hipError_t vcfc_subset_write(const VcfcSubsetArgs &a, uint64_t first, uint64_t last, hipStream_t s) {
    if (last <= first) return hipSuccess;
    const uint64_t per_block = SUB_WAVES * (a.select ? SEL_R : 1);
    const dim3 grid((unsigned)((last - first + per_block - 1) / per_block)), block(64 * SUB_WAVES);
    if (a.select) hipLaunchKernelGGL(k_sub_write<true>, grid, block, 0, s, a, first, last);
    else hipLaunchKernelGGL(k_sub_write<false>, grid, block, 0, s, a, first, last);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sub_wseq, dim3(VCFC_SUBSET_SEQ_LANES / 64), dim3(64), 0, s, a, first, last);
    return hipGetLastError();
}
