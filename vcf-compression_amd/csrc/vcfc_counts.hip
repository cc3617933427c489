// vcfc_counts.hip -- gfx950 kernels of genotype-counts: per
// record the eight counters n00 n01 n10 n11 n_other AN AC1 AC_other, per
// sample the five class counters, both read off the run-length code: a run
// byte is a count, and its place in the prefix sum over run counts is the
// column range it covers.  Every record is read once.
//
//   k_cnt_scan    a resident grid (a few blocks per CU); a block owns (sample
//                 table asked for, S <= VCFC_COUNTS_LDS_SAMPLES) an LDS tile
//                 hist[4][S] of uint32: c01 c10 c11 c_other, class-major, and
//                 its waves take chunks of 16 consecutive records, dealt
//                 round-robin over the grid.  One wave per record: header, REQ
//                 and the closing LF are checked, the sample section is
//                 scanned in 256-byte windows (scan_window, shared with the
//                 decoder) and every item start that is not a 0|0 run is
//                 counted: the class runs' counts of a lane's four bytes go to
//                 the record's counters by v_dot4_u32_u8, and each run adds 1
//                 to columns [a, a + c) of its class with LDS atomics (a
//                 per-lane loop); an escape's 3-byte token is classified and
//                 GT-parsed from its payload.  0|0 runs cost
//                 nothing beyond the scan: n00 and c00 are what is left of S
//                 and of the counted records.  A record that is not "simple"
//                 (the decoder's sense) takes back what it added to the tile
//                 and is queued.  The block flushes the tile's non-zero words
//                 once, with global atomics into the call's uint64 table.
//   k_cnt_seq     one lane per queued record: the byte-serial walk of a
//                 regular record (its row, its columns by global atomics, or
//                 error code 3).
//   k_cnt_finish  the call's table into the caller's: c00 = counted records -
//                 the other four; [4][S] -> [S][5], added.
//
// 32-bit counters: S < 2^30 and a record below 2^31 bytes give AN <= 2 S +
// (bytes of escaped tokens) < 2^32; a tile word counts at most the records of
// one call (< 2^32).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vcfc_wave.h>   // angle brackets: tests/simt_emu shadows it
#include "vcfc_device.h"
#include "vcfc_decode_dev.h"

namespace {

constexpr int CNT_WAVES = 8;          // waves per block
constexpr uint32_t CNT_CH = 16;       // consecutive records a wave takes at a time
constexpr uint32_t CNT_TILE = 4 * VCFC_COUNTS_LDS_SAMPLES;   // words of the LDS tile

constexpr int H_NONE = 0, H_LDS = 1, H_GLOBAL = 2;   // no sample table | LDS tile | global atomics

// Class of a token: 0..3 = exactly 0|0 0|1 1|0 1|1, 4 = anything else; and
// its GT subfield's called alleles (GT ends at the first ':',
// pieces split at '|' and '/', a piece of digits is an allele of class
// min(2, value)).  at(k): byte k of the token.
template <class F>
__device__ __forceinline__ uint32_t tok_count(F at, uint32_t len, uint32_t &an, uint32_t &ac1, uint32_t &aco) {
    uint32_t v = 0;
    bool digits = false, other = false;
    for (uint32_t k = 0;; k++) {
        const uint32_t b = k < len ? at(k) : ':';
        if (b == ':' || b == '|' || b == '/') {
            if (digits && !other) {
                an++;
                ac1 += v == 1;
                aco += v == 2;
            }
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
    if (len != 3 || at(1) != '|') return 4u;
    const uint32_t x = at(0) - '0', y = at(2) - '0';
    return x < 2u && y < 2u ? 2u * x + y : 4u;
}

// hist word of class k (1..4) and column col, += d (1, or ~0 to take it back)
template <int HIST>
__device__ __forceinline__ void hist_add(const VcfcCountsArgs &a, uint32_t *tile, uint32_t k, uint32_t col, uint32_t d) {
    const uint64_t w = (uint64_t)(k - 1) * a.S + col;
    if (HIST == H_LDS) atomicAdd(tile + (uint32_t)w, d);
    else if (HIST == H_GLOBAL)
        atomicAdd((unsigned long long *)a.hist + w, (unsigned long long)(long long)(int32_t)d);
}

// a lane's share of a record's counters.  an ac1 aco: the called alleles of
// the n_other tokens alone; a token of class 0..3 has the two its class says.
struct Acc {
    uint32_t n01 = 0, n10 = 0, n11 = 0, nother = 0, an = 0, ac1 = 0, aco = 0;
};

// The sample items [s0, s1) of a staged record, windows before `limit`: every
// item start that is not a 0|0 run into acc and (HIST) the histogram, by d.
// Stops at the first window that is not simple or passes S: its position (no
// item of it counted), else ~0u.
template <int HIST>
__device__ __forceinline__ uint32_t scan_items(const VcfcCountsArgs &a, Staged &sg, uint32_t s0, uint32_t s1,
                                               uint32_t limit, uint32_t d, uint32_t *tile, Acc &acc,
                                               uint32_t *got) {
    const uint32_t l = vw::lane_id();
    ItemState st;
    uint32_t stop = ~0u;
    for (uint32_t cur = s0 & ~3u; cur < s1 && cur < limit; cur += 256) {
        sg.need(cur, 256 + 8);
        const uint32_t b = umin32(cur + 256, s1);
        const uint32_t v4 = sg.at4(cur + 4 * l);
        const ItemLane it = scan_window(v4, cur, s0, b, s1, st);
        if (st.bad || st.got > a.S) {
            stop = cur;
            break;
        }
        const uint32_t hi = msb4(v4) & it.start;   // class runs and escapes
        if (vw::ballot(hi != 0) == 0) continue;    // a window of 0|0 runs
        // the lane's four bytes at once: 0x01 in the bytes that start a run of
        // each class (bits 6 5 of the byte: 00 = 1|1, 01 = 0|1, 10 = 1|0, 11 =
        // escape), their counts summed by v_dot4_u32_u8
        const uint32_t h1 = vw::umul24(hi, 0x00204081u) & 0x01010101u;
        const uint32_t b5 = (v4 >> 5) & h1, b6 = (v4 >> 6) & h1;
        const uint32_t c8 = v4 & 0x1F1F1F1Fu;
        const uint32_t esc = b5 & b6;
        acc.n01 = vw::dot4u(c8, b5 & ~b6, acc.n01);
        acc.n10 = vw::dot4u(c8, b6 & ~b5, acc.n10);
        acc.n11 = vw::dot4u(c8, h1 & ~(b5 | b6), acc.n11);
        if (vw::ballot(esc != 0)) {   // (simple: 3 payload bytes and a TAB, inside the record)
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                if (!((esc >> (8 * j)) & 1u)) continue;
                const uint32_t p = cur + 4 * l + j;
                const uint32_t w = sg.at(p + 1) | (sg.at(p + 2) << 8) | (sg.at(p + 3) << 16);
                uint32_t an = 0, ac1 = 0, aco = 0;
                const uint32_t k = tok_count([&](uint32_t q) { return (w >> (8 * q)) & 0xFFu; }, 3u, an, ac1, aco);
                acc.n01 += k == 1;
                acc.n10 += k == 2;
                acc.n11 += k == 3;
                if (k == 4) {
                    acc.nother++;
                    acc.an += an;
                    acc.ac1 += ac1;
                    acc.aco += aco;
                }
                if (HIST != H_NONE && k) hist_add<HIST>(a, tile, k, it.gb[j], d);
            }
        }
        if (HIST == H_NONE) continue;
        const uint32_t run = h1 & ~esc;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            if (!((run >> (8 * j)) & 1u)) continue;
            const uint32_t bt = v4 >> (8 * j), m = bt & 0xE0u;   // 0|1 -> 0xA0, 1|0 -> 0xC0, 1|1 -> 0x80
            const uint32_t k = m == 0xA0u ? 1u : m == 0xC0u ? 2u : 3u, c = bt & 0x1Fu;
            for (uint32_t t = 0; t < c; t++) hist_add<HIST>(a, tile, k, it.gb[j] + t, d);
        }
    }
    *got = st.got;
    return stop;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return vw::readlane(vw::scan_add(v), 63); }

// One record, one wave.  false: not simple, nothing of it is left in the
// histogram and no row is written (the caller queues it).
template <int HIST>
__device__ __forceinline__ bool count_one(const VcfcCountsArgs &a, uint64_t i, uint8_t *sb, uint32_t *tile) {
    const uint32_t l = vw::lane_id();
    RecFrame f;
    if (!frame_open(f, sb, a.in, a.rec_start[i], a.rec_start[i + 1]) || f.slen != f.req) return false;   // (no NUL in REQ)
    Staged &sg = f.sg;
    const uint32_t s0 = f.s0(), s1 = f.s1();
    Acc acc;
    uint32_t got;
    const uint32_t stop = scan_items<HIST>(a, sg, s0, s1, ~0u, 1u, tile, acc, &got);
    if (stop != ~0u || got != a.S) {
        if (HIST != H_NONE) {   // take back the windows before the stop
            Acc unused;
            (void)scan_items<HIST>(a, sg, s0, s1, stop, ~0u, tile, unused, &got);
        }
        return false;
    }
    if (a.variant) {
        // the wave's sums, two to a register while every total stays below
        // 2^16 (each is at most 2 S); the n_other tokens' four only where there are any
        const uint32_t S = (uint32_t)a.S;
        const bool any_other = vw::ballot(acc.nother != 0) != 0;
        uint32_t n01, n10, n11, nother = 0, an = 0, ac1 = 0, aco = 0;
        if (S < (1u << 15)) {
            const uint32_t p0 = wave_sum(acc.n01 | (acc.n10 << 16));
            n01 = p0 & 0xFFFFu; n10 = p0 >> 16;
            if (any_other) {
                const uint32_t p1 = wave_sum(acc.n11 | (acc.nother << 16)), p2 = wave_sum(acc.an | (acc.ac1 << 16));
                n11 = p1 & 0xFFFFu; nother = p1 >> 16; an = p2 & 0xFFFFu; ac1 = p2 >> 16;
                aco = wave_sum(acc.aco);
            } else {
                n11 = wave_sum(acc.n11);
            }
        } else {
            n01 = wave_sum(acc.n01); n10 = wave_sum(acc.n10); n11 = wave_sum(acc.n11);
            if (any_other) {
                nother = wave_sum(acc.nother); an = wave_sum(acc.an); ac1 = wave_sum(acc.ac1); aco = wave_sum(acc.aco);
            }
        }
        if (l == 0) {
            uint4 *row = reinterpret_cast<uint4 *>(a.variant + 8 * i);
            row[0] = make_uint4(S - n01 - n10 - n11 - nother, n01, n10, n11);
            row[1] = make_uint4(nother, 2u * (S - nother) + an, n01 + n10 + 2u * n11 + ac1, aco);
        }
    }
    return true;
}

template <bool SEL, int HIST>
__global__ __launch_bounds__(64 * CNT_WAVES) void k_cnt_scan(VcfcCountsArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t sbuf[CNT_WAVES * SBUF];
    __shared__ uint32_t tile[HIST == H_LDS ? CNT_TILE : 4];
    const uint32_t words = 4u * (uint32_t)a.S;   // (H_LDS: S <= VCFC_COUNTS_LDS_SAMPLES)
    if (HIST == H_LDS) {
        for (uint32_t w = threadIdx.x; w < words; w += 64 * CNT_WAVES) tile[w] = 0;
        __syncthreads();
    }
    const uint32_t wave = vw::readfirst(threadIdx.x >> 6);
    const uint32_t l = vw::lane_id();
    uint8_t *sb = sbuf + wave * SBUF;
    uint32_t counted = 0;
    // chunks of CNT_CH consecutive records, dealt round-robin to the grid's
    // waves: the records a query selects are neighbours, and spread over all blocks
    const uint64_t stride = (uint64_t)gridDim.x * CNT_WAVES * CNT_CH;
    for (uint64_t c0 = ((uint64_t)blockIdx.x * CNT_WAVES + wave) * CNT_CH; c0 < a.n; c0 += stride) {
        const uint64_t il = c0 + l;
        const bool mine = l < CNT_CH && il < a.n;
        const bool on = mine && (!SEL || a.select[il]);
        if (SEL && a.variant && mine && !on) {
            uint4 *row = reinterpret_cast<uint4 *>(a.variant + 8 * il);
            row[0] = row[1] = make_uint4(0u, 0u, 0u, 0u);
        }
        const uint64_t m0 = vw::ballot(on);
        counted += (uint32_t)vw::popc64(m0);
        for (uint64_t m = m0; m; m &= m - 1) {
            const uint64_t i = c0 + (uint64_t)__builtin_ctzll(m);
            if (!count_one<HIST>(a, i, sb, tile) && l == 0) {
                const uint32_t q = atomicAdd(a.seq_count, 1u);
                a.seq_list[q] = (uint32_t)i;
            }
        }
    }
    if (l == 0 && counted) atomicAdd((unsigned long long *)a.counted, (unsigned long long)counted);
    if (HIST == H_LDS) {
        __syncthreads();
        for (uint32_t w = threadIdx.x; w < words; w += 64 * CNT_WAVES) {
            const uint32_t v = tile[w];
            if (v) atomicAdd((unsigned long long *)a.hist + w, (unsigned long long)v);
        }
    }
}

// The byte-serial walk of a regular record (walk_regular, vcfc_decode_dev.h)
// [rs, re): its row and (HIST) its columns; false where the record is not
// regular (the row is not written; the table is not meaningful then).  (The
// walk's length bound is the 32-bit counters' bound, see above.)
template <bool HIST>
__device__ bool cnt_walk(const VcfcCountsArgs &a, uint64_t i, uint64_t rs, uint64_t re) {
    const uint8_t *in = a.in;
    uint32_t n01 = 0, n10 = 0, n11 = 0, nother = 0, nesc = 0, an = 0, ac1 = 0, aco = 0;
    const bool ok = walk_regular<true>(
        in, rs, re, a.S,
        [&](uint64_t got, const uint8_t *src, uint32_t len) {
            const uint32_t k = tok_count([&](uint32_t q) { return (uint32_t)src[q]; }, len, an, ac1, aco);
            nesc++;
            n01 += k == 1;
            n10 += k == 2;
            n11 += k == 3;
            nother += k == 4;
            if (HIST && k) hist_add<H_GLOBAL>(a, nullptr, k, (uint32_t)got, 1u);
        },
        [&](uint8_t b, uint64_t got, uint32_t cnt) {
            if (b < 0x80u) return;   // a 0|0 run
            const uint32_t m = b & 0xE0u;
            const uint32_t k = m == 0xA0u ? 1u : m == 0xC0u ? 2u : 3u;
            n01 += k == 1 ? cnt : 0u;
            n10 += k == 2 ? cnt : 0u;
            n11 += k == 3 ? cnt : 0u;
            ac1 += k == 3 ? 2 * cnt : cnt;
            if (HIST)
                for (uint32_t t = 0; t < cnt; t++) hist_add<H_GLOBAL>(a, nullptr, k, (uint32_t)got + t, 1u);
        });
    if (!ok) return false;
    if (a.variant) {
        uint32_t *row = a.variant + 8 * i;
        const uint32_t S32 = (uint32_t)a.S;
        row[0] = S32 - n01 - n10 - n11 - nother; row[1] = n01; row[2] = n10; row[3] = n11;
        row[4] = nother; row[5] = 2u * (S32 - nesc) + an; row[6] = ac1; row[7] = aco;
    }
    return true;
}

// Queued records, one lane each (grid-stride).
template <bool HIST>
__global__ __launch_bounds__(256) void k_cnt_seq(VcfcCountsArgs a) {
    const uint32_t cnt = *a.seq_count;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < cnt; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = a.seq_list[q];
        if (!cnt_walk<HIST>(a, i, a.rec_start[i], a.rec_start[i + 1]))
            atomicMin((unsigned long long *)a.err, (unsigned long long)((i << 8) | 3u));
    }
}

__global__ __launch_bounds__(256) void k_cnt_finish(VcfcCountsArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.S) return;
    const uint64_t c01 = a.hist[j], c10 = a.hist[a.S + j], c11 = a.hist[2 * a.S + j], co = a.hist[3 * a.S + j];
    uint64_t *o = a.sample + 5 * j;
    o[0] += *a.counted - c01 - c10 - c11 - co;
    o[1] += c01;
    o[2] += c10;
    o[3] += c11;
    o[4] += co;
}

__global__ void k_cnt_reset(uint64_t *err, uint32_t *seq_count, uint64_t *counted) {
    if (threadIdx.x == 0) {
        *err = ~0ull;
        *seq_count = 0;
        *counted = 0;
    }
}

template <bool SEL, int HIST>
void launch_scan(const VcfcCountsArgs &a, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL((k_cnt_scan<SEL, HIST>), dim3(blocks), dim3(64 * CNT_WAVES), 0, s, a);
}

// the histogram k_cnt_scan is launched with
int hist_of(uint64_t S, bool with_sample_table) {
    return !with_sample_table ? H_NONE : S <= VCFC_COUNTS_LDS_SAMPLES ? H_LDS : H_GLOBAL;
}

// as many blocks of k_cnt_scan as stay resident on the current device (two
// per CU with the tile, four without), so each tile is flushed once over many
// records
hipError_t resident_blocks(int hist, uint64_t *blocks) {
    int dev = 0, cus = 0;
    hipError_t e;
    if ((e = hipGetDevice(&dev)) != hipSuccess ||
        (e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess)
        return e;
    *blocks = (hist == H_LDS ? 2ull : 4ull) * (uint64_t)(cus > 0 ? cus : 1);
    return hipSuccess;
}

}  // namespace

uint64_t vcfc_counts_scan_trip(uint64_t S, bool with_sample_table) {
    uint64_t blocks = 0;
    if (resident_blocks(hist_of(S, with_sample_table), &blocks) != hipSuccess) return 0;
    return blocks * CNT_WAVES * CNT_CH;
}

VcfcCountsLayout vcfc_counts_workspace_layout(uint64_t n, uint64_t S) {
    auto al = [](uint64_t x) { return (x + 255) & ~255ull; };
    VcfcCountsLayout L;
    uint64_t o = 0;
    L.hist = o; o = al(o + 32 * S);
    L.counted = o; o = al(o + 8);
    L.seq_list = o; o = al(o + 4 * (n + 1));
    L.seq_count = o; o = al(o + 8);
    L.err = o; o = al(o + 8);
    L.total = o;
    return L;
}

hipError_t vcfc_counts_run(const VcfcCountsArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_cnt_reset, dim3(1), dim3(64), 0, s, a.err, a.seq_count, a.counted);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.n == 0) return e;
    if (a.sample && (e = hipMemsetAsync(a.hist, 0, 32 * a.S, s)) != hipSuccess) return e;
    const uint64_t chunk = (uint64_t)CNT_WAVES * CNT_CH;
    const int hist = hist_of(a.S, a.sample != nullptr);
    uint64_t max_blocks = 0;
    if ((e = resident_blocks(hist, &max_blocks)) != hipSuccess) return e;
    const uint64_t blocks = std::min<uint64_t>(max_blocks, (a.n + chunk - 1) / chunk);
    const unsigned g = (unsigned)blocks;
    if (a.select) {
        if (hist == H_NONE) launch_scan<true, H_NONE>(a, g, s);
        else if (hist == H_LDS) launch_scan<true, H_LDS>(a, g, s);
        else launch_scan<true, H_GLOBAL>(a, g, s);
    } else {
        if (hist == H_NONE) launch_scan<false, H_NONE>(a, g, s);
        else if (hist == H_LDS) launch_scan<false, H_LDS>(a, g, s);
        else launch_scan<false, H_GLOBAL>(a, g, s);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint64_t want = (a.n + 255) / 256;
    const dim3 sg((unsigned)(want < 1024 ? want : 1024));
    if (a.sample) hipLaunchKernelGGL(k_cnt_seq<true>, sg, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_cnt_seq<false>, sg, dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess || !a.sample) return e;
    hipLaunchKernelGGL(k_cnt_finish, dim3((unsigned)((a.S + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
