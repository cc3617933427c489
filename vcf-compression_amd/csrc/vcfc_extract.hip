// vcfc_extract.hip -- gfx950 kernels of extract: REQ and K
// chosen sample columns of every record, written as a .vcfc record again.  The
// chosen tokens are found as the sample-subset decoder finds them
// (vcfc_subset.hip, §4i) and re-run-length-coded where they are: a record
// never becomes text.
//
//   k_ex_plan   one wave per record: a simple record (the decoder's sense)
//               whose REQ holds no NUL, with K <= VCFC_EXTRACT_TILE and at
//               most EX_OTH chosen tokens outside the four classes, is sized
//               exactly: its chosen tokens are resolved into a tile of class
//               bytes in LDS and the tile is re-coded (recode_tile).  Others
//               are queued.
//   k_ex_seq    a fixed number of lanes over the queue: the byte-serial walk
//               of a regular record and the serial re-code (size, or error
//               code 3 / 5).
//   scan        record offsets (the encoder's exclusive scan).
//   k_ex_write  one wave per record, simple records: the same resolve and
//               re-code, now storing the record's bytes at its offset.
//   k_ex_wseq   the queued regular records, one lane each.
//
// The plan is exact (every record is read twice), so one call gives exact
// record offsets with no host round trip, as in §4i.
#include <hip/hip_runtime.h>
#include <vcfc_wave.h>   // angle brackets: tests/simt_emu shadows it
#include "vcfc_device.h"
#include "vcfc_decode_dev.h"

namespace {

constexpr int EX_WAVES = 4;                      // records per 256-thread block
constexpr uint32_t EX_TK = VCFC_EXTRACT_TILE;    // class bytes of the LDS tile per wave
constexpr uint32_t EX_TK_SMALL = 512;            // the tile of a call with K <= 512
constexpr uint32_t EX_OTH = 248;                 // other tokens a tile byte can name (4 + index <= 251)
constexpr uint32_t EX_CODE5_LEN = 1u << 30;      // a record's LEN field holds 30 bits

constexpr uint32_t XS_SIMPLE = 0;     // wave-parallel
constexpr uint32_t XS_SEQ = 1;        // regular, byte-serial
constexpr uint32_t XS_ERR = 3;        // not regular, or not re-encodable: no record
constexpr uint32_t XS_SKIP = 5;       // not selected: no record

// Token classes: 2 a + b for the token "a|b" (a, b in {0, 1}); 4 and above:
// any other token.  The run byte of a class: its code, plus the count.
__device__ __forceinline__ uint32_t class_code(uint32_t cls) {
    return cls == 0 ? 0x00u : cls == 1 ? 0xA0u : cls == 2 ? 0xC0u : 0x80u;
}
__device__ __forceinline__ uint32_t class_cap(uint32_t cls) { return cls == 0 ? 127u : 31u; }
__device__ __forceinline__ uint32_t class_of_run(uint32_t b) {
    const uint32_t m = b & 0xE0u;
    return b < 0x80u ? 0u : m == 0xA0u ? 1u : m == 0xC0u ? 2u : 3u;
}
// the class a 3-byte token spells (b0 | b1 << 8 | b2 << 16), or 4
__device__ __forceinline__ uint32_t class_of_word(uint32_t w) {
    const uint32_t x = (w & 0x00FFFFFFu) ^ 0x00307C30u;   // "0|0"
    return (x & ~0x00010001u) ? 4u : ((x & 1u) << 1) | (x >> 16);
}

__device__ __forceinline__ void put_be30(uint8_t *h, uint32_t v) {
    h[0] = (uint8_t)(0xC0u | (v >> 24));
    h[1] = (uint8_t)(v >> 16);
    h[2] = (uint8_t)(v >> 8);
    h[3] = (uint8_t)v;
}

// ---- the wave path ----------------------------------------------------------

// REQ of the staged frame can be encoded again: its first byte is neither TAB
// nor '#', its last byte is a TAB, no two TABs are adjacent.
__device__ __forceinline__ bool req_encodable(RecFrame &f) {
    const uint32_t l = vw::lane_id();
    const uint32_t r0 = f.rs + 8, req = f.req;
    uint32_t carry = 0;   // the byte before this step's first
    bool bad = false;
    for (uint32_t b0 = 0; b0 < req; b0 += 64) {
        f.sg.need(r0 + b0);
        const uint32_t k = b0 + l;
        const uint32_t b = k < req ? f.sg.at(r0 + k) : 0u;
        const uint32_t pb = vw::shr1(b, carry);
        carry = vw::readlane(b, 63);
        const bool x = k < req && ((k == 0 && (b == '\t' || b == '#')) || (k > 0 && b == '\t' && pb == '\t') ||
                                   (k + 1 == req && b != '\t'));
        bad = bad || vw::ballot(x) != 0;
    }
    return !bad;
}

// The chosen tokens of the frame's sample items into the tile: T[r] = class of
// the token at output slot r, or 4 + j with its three bytes in O[j].  CHECK:
// every window is scanned (is the record simple?); else the scan stops with
// the last chosen column.  Returns the scan's state; *noth = other tokens met
// (those past EX_OTH are counted, not kept).
template <bool CHECK>
__device__ __forceinline__ ItemState resolve_tile(const VcfcExtractArgs &a, RecFrame &f, uint32_t tq, uint32_t rq,
                                                  uint32_t *G, uint8_t *T, uint32_t *O, uint32_t *noth) {
    const uint32_t l = vw::lane_id();
    const uint32_t K = a.K;
    Staged &sg = f.sg;
    const uint32_t s0 = f.s0(), s1 = f.s1();
    ItemState st;
    uint32_t c = 0, no = 0;                  // cursor into csort, other tokens so far (wave-uniform)
    uint32_t nextt = vw::readlane(tq, 0);    // csort[c]
    for (uint32_t cur = s0 & ~3u; cur < s1 && (CHECK ? !st.bad : c < K); cur += 256) {
        sg.need(cur, 256 + 8);
        const uint32_t b = umin32(cur + 256, s1);
        const ItemLane it = scan_window(sg.at4(cur + 4 * l), cur, s0, b, s1, st);
        if (nextt >= st.got) continue;   // no chosen column in this window
        // G[k] = tokens before byte k's item (k_sub_write's search, §4i)
        vw::wave_sync();
        *reinterpret_cast<uint4 *>(G + 4 * l) = make_uint4(it.gb[0], it.gb[1], it.gb[2], it.gb[3]);
        vw::wave_sync();
        for (;;) {
            const uint32_t t = tq;
            const bool in_win = t < st.got;   // (ascending: the lanes that hold one are the first ones)
            uint32_t cls = 0, w = 0;
            if (in_win) {
                uint32_t lo = 0;
#pragma unroll
                for (uint32_t step = 128; step; step >>= 1)
                    if (G[lo + step] <= t) lo += step;
                const uint32_t p = cur + lo;
                const uint32_t bt = sg.at(p);
                if (bt == 0xE1u) {
                    w = sg.at(p + 1) | (sg.at(p + 2) << 8) | (sg.at(p + 3) << 16);
                    cls = class_of_word(w);   // an escape that spells a class joins its run
                } else {
                    cls = class_of_run(bt);
                }
            }
            const uint64_t om = vw::ballot(in_win && cls == 4);
            if (in_win) {
                if (cls == 4) {
                    const uint32_t j = no + (uint32_t)vw::popc64(om & vw::lanemask_lt());
                    if (j < EX_OTH) O[j] = w;
                    cls = 4 + umin32(j, EX_OTH - 1);
                }
                T[rq] = (uint8_t)cls;
            }
            no += (uint32_t)vw::popc64(om);
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
    vw::wave_sync();
    *noth = no;
    return st;
}

// The tile re-coded greedily in output order: the bytes of the record's
// sample section (WRITE: stored at dst).  Slot r lies p slots into its run (a
// run starts where the class changes, and at every other token; the last
// start comes from a ballot, carried across the 64-slot batches); the slot
// that fills a run byte, or ends the run, emits that byte: full bytes first,
// the remainder last.  Another token emits 0xE1, its bytes and -- unless it is
// the last slot -- a TAB.
template <bool WRITE>
__device__ __forceinline__ uint32_t recode_tile(uint32_t K, const uint8_t *T, const uint32_t *O, uint8_t *dst) {
    const uint32_t l = vw::lane_id();
    const uint64_t le = l == 63 ? ~0ull : (2ull << l) - 1;   // lanes <= l
    uint32_t off = 0, start_carry = 0;
    for (uint32_t r0 = 0; r0 < K; r0 += 64) {
        const uint32_t r = r0 + l;
        const bool in = r < K;
        const uint32_t cls = in ? T[r] : 0xFFu;
        const uint32_t prev = in && r > 0 ? T[r - 1] : 0xFEu;
        const uint32_t next = r + 1 < K ? T[r + 1] : 0xFEu;
        const uint64_t sm = vw::ballot(in && (cls >= 4 || cls != prev));
        const uint32_t start = (sm & le) ? r0 + (uint32_t)vw::hibit64(sm & le) : start_carry;
        if (sm) start_carry = r0 + (uint32_t)vw::hibit64(sm);
        uint32_t n = 0, val = 0;
        if (in) {
            if (cls >= 4) {
                n = r + 1 == K ? 4u : 5u;
            } else {
                const uint32_t p = r - start;
                const uint32_t q = cls == 0 ? p % 127u : p % 31u;
                n = next != cls || q + 1 == class_cap(cls);
                val = class_code(cls) | (q + 1);
            }
        }
        if (!WRITE) {   // sizing: the batch's bytes, no offsets
            off += (uint32_t)vw::popc64(vw::ballot(n == 1)) + 4u * (uint32_t)vw::popc64(vw::ballot(n >= 4)) +
                   (uint32_t)vw::popc64(vw::ballot(n == 5));
            continue;
        }
        const uint32_t inc = vw::scan_add(n);
        if (n) {
            uint8_t *o = dst + (off + inc - n);
            if (cls < 4) {
                o[0] = (uint8_t)val;
            } else {
                const uint32_t w = O[cls - 4];
                o[0] = 0xE1u;
                o[1] = (uint8_t)w;
                o[2] = (uint8_t)(w >> 8);
                o[3] = (uint8_t)(w >> 16);
                if (n == 5) o[4] = '\t';
            }
        }
        off += vw::readlane(inc, 63);
    }
    return off;
}

// One record, one wave: sized on the wave path, refused (code 5), or queued.
__device__ __forceinline__ void plan_one(const VcfcExtractArgs &a, uint64_t i, uint8_t *sb, uint32_t *G, uint8_t *T,
                                         uint32_t *O) {
    const uint32_t l = vw::lane_id();
    const uint32_t K = a.K;
    const uint64_t rs_abs = a.rec_start[i], re_abs = a.rec_start[i + 1];
    bool simple = false, enc = false;
    uint64_t size = 0;
    RecFrame f;
    if (K <= EX_TK) {
        const uint32_t tq = l < K ? a.csort[l] : ~0u, rq = l < K ? a.rank[l] : 0u;
        if (frame_open(f, sb, a.in, rs_abs, re_abs) && f.slen == f.req) {   // (no NUL in REQ)
            enc = req_encodable(f);
            uint32_t noth;
            const ItemState st = resolve_tile<true>(a, f, tq, rq, G, T, O, &noth);
            simple = !st.bad && st.got == a.S && noth <= EX_OTH;
            if (simple && enc) {
                size = 9ull + f.req + recode_tile<false>(K, T, O, nullptr);
                enc = size - 4 < EX_CODE5_LEN;
            }
            vw::wave_sync();   // T and O are free for the wave's next record
        }
    }
    if (l == 0) {
        a.st[i] = !simple ? XS_SEQ : enc ? XS_SIMPLE : XS_ERR;
        a.line_size[i] = simple && enc ? (uint32_t)size : 0u;
        if (!simple) {
            const uint32_t q = atomicAdd(a.seq_count, 1u);
            a.seq_list[q] = (uint32_t)i;
        } else if (!enc) {
            atomicMin((unsigned long long *)a.err, (unsigned long long)((i << 8) | 5u));
        }
    }
}

// (selected mode, a.select set: the dealing of SEL_R records to a wave,
// vcfc_decode_dev.h)
// (TK: the tile's bytes per wave -- EX_TK_SMALL while K fits, for occupancy)
template <bool SEL, uint32_t TK>
__global__ __launch_bounds__(256) void k_ex_plan(VcfcExtractArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t sbuf[EX_WAVES * SBUF];
    __shared__ __attribute__((aligned(16))) uint32_t gbuf[EX_WAVES * 256];
    __shared__ __attribute__((aligned(16))) uint8_t tbuf[EX_WAVES * TK];
    __shared__ __attribute__((aligned(16))) uint32_t obuf[EX_WAVES * EX_OTH];
    const uint32_t wave = vw::readfirst(threadIdx.x >> 6);
    uint8_t *sb = sbuf + wave * SBUF;
    uint32_t *G = gbuf + wave * 256;
    uint8_t *T = tbuf + wave * TK;
    uint32_t *O = obuf + wave * EX_OTH;
    const uint64_t g = (uint64_t)blockIdx.x * EX_WAVES + wave;
    if (!SEL) {
        if (g < a.n) plan_one(a, g, sb, G, T, O);
        return;
    }
    const uint64_t Gw = (uint64_t)gridDim.x * EX_WAVES;
    const uint32_t l = vw::lane_id();
    const uint64_t il = g + (uint64_t)l * Gw;
    const bool mine = l < SEL_R && il < a.n;
    const bool on = mine && a.select[il];
    if (mine && !on) { a.st[il] = XS_SKIP; a.line_size[il] = 0; }
    for (uint64_t m = vw::ballot(on); m; m &= m - 1)
        plan_one(a, g + (uint64_t)__builtin_ctzll(m) * Gw, sb, G, T, O);
}

// Simple record i written at out + line_off[i]: both headers, REQ verbatim,
// the re-coded sample section, the LF.
__device__ __forceinline__ void write_one(const VcfcExtractArgs &a, uint64_t i, uint8_t *sb, uint32_t *G, uint8_t *T,
                                          uint32_t *O) {
    const uint32_t l = vw::lane_id();
    const uint32_t K = a.K;
    const uint64_t L0 = a.line_off[i], L1 = a.line_off[i + 1];
    const uint32_t rst = a.st[i];
    const uint64_t rs_abs = a.rec_start[i], re_abs = a.rec_start[i + 1];
    const uint32_t tq = l < K ? a.csort[l] : ~0u, rq = l < K ? a.rank[l] : 0u;
    if (L1 > a.out_cap) {
        if (l == 0) atomicMin((unsigned long long *)a.err, (unsigned long long)((i << 8) | 0xFFu));
        return;
    }
    if (rst != XS_SIMPLE) return;   // queued records: k_ex_wseq; no record otherwise
    RecFrame f;
    frame_stage(f, sb, a.in, rs_abs, re_abs);
    Staged &sg = f.sg;
    const uint32_t rs = f.rs, req = f.req;
    uint8_t *rec = a.out + L0;
    if (l == 0) {
        put_be30(rec, (uint32_t)(L1 - L0 - 4));
        put_be30(rec + 4, req);
        rec[L1 - L0 - 1] = '\n';
    }
    // REQ verbatim (4 bytes per lane, 256 per step)
    for (uint32_t b0 = 0; b0 < req; b0 += 256) {
        sg.need(rs + 8 + b0, 256);
        const uint32_t k = b0 + 4 * l;
        if (k < req) {
            uint32_t w;
            __builtin_memcpy(&w, sg.lds + (rs + 8 + k - sg.cbase), 4);   // (unaligned ds_read_b32)
            if (k + 4 <= req) {
                __builtin_memcpy(rec + 8 + k, &w, 4);
            } else {
                for (uint32_t j = 0; j < 3; j++)
                    if (k + j < req) rec[8 + k + j] = (uint8_t)(w >> (8 * j));
            }
        }
    }
    uint32_t noth;
    (void)resolve_tile<false>(a, f, tq, rq, G, T, O, &noth);
    (void)recode_tile<true>(K, T, O, rec + 8 + req);
    vw::wave_sync();   // T and O are free for the wave's next record
}

template <bool SEL, uint32_t TK>
__global__ __launch_bounds__(256) void k_ex_write(VcfcExtractArgs a, uint64_t first, uint64_t last) {
    __shared__ __attribute__((aligned(16))) uint8_t sbuf[EX_WAVES * SBUF];
    __shared__ __attribute__((aligned(16))) uint32_t gbuf[EX_WAVES * 256];
    __shared__ __attribute__((aligned(16))) uint8_t tbuf[EX_WAVES * TK];
    __shared__ __attribute__((aligned(16))) uint32_t obuf[EX_WAVES * EX_OTH];
    const uint32_t wave = vw::readfirst(threadIdx.x >> 6);
    uint8_t *sb = sbuf + wave * SBUF;
    uint32_t *G = gbuf + wave * 256;
    uint8_t *T = tbuf + wave * TK;
    uint32_t *O = obuf + wave * EX_OTH;
    const uint64_t g = (uint64_t)blockIdx.x * EX_WAVES + wave;
    if (!SEL) {
        if (first + g < last) write_one(a, first + g, sb, G, T, O);
        return;
    }
    const uint64_t Gw = (uint64_t)gridDim.x * EX_WAVES;
    const uint32_t l = vw::lane_id();
    const uint64_t il = first + g + (uint64_t)l * Gw;
    const bool cand = l < SEL_R && il < last;
    for (uint64_t m = vw::ballot(cand && a.select[il]); m; m &= m - 1)
        write_one(a, first + g + (uint64_t)__builtin_ctzll(m) * Gw, sb, G, T, O);
}

// ---- the byte-serial path -----------------------------------------------------

// The byte-serial walk of a regular record (walk_regular, vcfc_decode_dev.h)
// [rs, re): false where the record is not regular.  scr[2 r], scr[2 r + 1]:
// the chosen token of output slot r, as (0x80000000 | class, 3) out of a run
// byte, else (its offset from rs, its length).  *empty: a chosen token is
// empty.
__device__ bool seq_walk(const VcfcExtractArgs &a, uint64_t rs, uint64_t re, uint32_t *scr, bool *empty) {
    uint32_t c = 0;
    const uint32_t K = a.K;
    bool em = false;
    const bool ok = walk_regular<true>(
        a.in, rs, re, a.S,
        [&](uint64_t got, const uint8_t *src, uint32_t len) {
            if (c < K && a.csort[c] == got) {
                const uint32_t r = a.rank[c++];
                scr[2 * r] = (uint32_t)(src - (a.in + rs));
                scr[2 * r + 1] = len;
                em = em || len == 0;
            }
        },
        [&](uint8_t b, uint64_t got, uint32_t cnt) {
            while (c < K && a.csort[c] < got + cnt) {
                const uint32_t r = a.rank[c++];
                scr[2 * r] = 0x80000000u | class_of_run(b);
                scr[2 * r + 1] = 3;
            }
        });
    *empty = em;
    return ok;
}

// The serial re-code of the K tokens seq_walk left in scr: the bytes of the
// sample section (WRITE: stored at dst).
template <bool WRITE>
__device__ uint64_t seq_recode(const VcfcExtractArgs &a, uint64_t rs, const uint32_t *scr, uint8_t *dst) {
    const uint32_t K = a.K;
    uint64_t o = 0;
    uint32_t cur = 4, cnt = 0;
    auto flush = [&]() {
        if (cnt) {
            if (WRITE) dst[o] = (uint8_t)(class_code(cur) | cnt);
            o++;
            cnt = 0;
        }
    };
    for (uint32_t r = 0; r < K; r++) {
        const uint32_t w = scr[2 * r], len = scr[2 * r + 1];
        const uint8_t *src = a.in + rs + (w & 0x7FFFFFFFu);
        uint32_t cls = 4;
        if (w & 0x80000000u) cls = w & 3u;
        else if (len == 3) cls = class_of_word(src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16));
        if (cls < 4) {
            if (cls != cur) {
                flush();
                cur = cls;
            }
            if (++cnt == class_cap(cls)) flush();
        } else {
            flush();
            cur = 4;
            if (WRITE) {
                dst[o] = 0xE1u;
                for (uint32_t k = 0; k < len; k++) dst[o + 1 + k] = src[k];
                if (r + 1 < K) dst[o + 1 + len] = '\t';
            }
            o += 1ull + len + (r + 1 < K);
        }
    }
    flush();
    return o;
}

__device__ bool seq_req_encodable(const uint8_t *req, uint32_t n) {
    if (req[0] == '\t' || req[0] == '#' || req[n - 1] != '\t') return false;
    for (uint32_t k = 1; k < n; k++)
        if (req[k] == '\t' && req[k - 1] == '\t') return false;
    return true;
}

// Queued records, a fixed number of lanes (lane t owns seq_scratch[2 t K,
// 2 (t + 1) K)).
__global__ __launch_bounds__(64) void k_ex_seq(VcfcExtractArgs a) {
    const uint32_t cnt = *a.seq_count;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t *scr = a.seq_scratch + 2 * t * a.K;
    for (uint64_t q = t; q < cnt; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = a.seq_list[q];
        const uint64_t rs = a.rec_start[i], re = a.rec_start[i + 1];
        bool empty = false;
        uint32_t code = 3;
        uint64_t size = 0;
        if (seq_walk(a, rs, re, scr, &empty)) {
            const uint32_t req = be30(a.in + rs + 4);
            code = 5;
            if (!empty && seq_req_encodable(a.in + rs + 8, req)) {
                size = 9ull + req + seq_recode<false>(a, rs, scr, nullptr);
                if (size - 4 < EX_CODE5_LEN) code = 0;
            }
        }
        a.st[i] = code ? XS_ERR : XS_SEQ;
        a.line_size[i] = code ? 0u : (uint32_t)size;
        if (code) atomicMin((unsigned long long *)a.err, (unsigned long long)((i << 8) | code));
    }
}

// The queued regular records of [first, last), one lane each.
__global__ __launch_bounds__(64) void k_ex_wseq(VcfcExtractArgs a, uint64_t first, uint64_t last) {
    const uint32_t cnt = *a.seq_count;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t *scr = a.seq_scratch + 2 * t * a.K;
    for (uint64_t q = t; q < cnt; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = a.seq_list[q];
        if (i < first || i >= last || a.st[i] != XS_SEQ) continue;
        const uint64_t L0 = a.line_off[i], L1 = a.line_off[i + 1];
        if (L1 > a.out_cap) {
            atomicMin((unsigned long long *)a.err, (unsigned long long)((i << 8) | 0xFFu));
            continue;
        }
        const uint64_t rs = a.rec_start[i], re = a.rec_start[i + 1];
        bool empty;
        if (!seq_walk(a, rs, re, scr, &empty)) continue;   // (the plan found it regular)
        const uint8_t *h = a.in + rs;
        const uint32_t req = be30(h + 4);
        uint8_t *rec = a.out + L0;
        put_be30(rec, (uint32_t)(L1 - L0 - 4));
        put_be30(rec + 4, req);
        for (uint32_t k = 0; k < req; k++) rec[8 + k] = h[8 + k];
        (void)seq_recode<true>(a, rs, scr, rec + 8 + req);
        rec[L1 - L0 - 1] = '\n';
    }
}

__global__ void k_ex_reset(uint64_t *err, uint32_t *seq_count, uint64_t *line_off0) {
    if (threadIdx.x == 0) {
        *err = ~0ull;
        *seq_count = 0;
        if (line_off0) *line_off0 = 0;
    }
}

}  // namespace

VcfcSubsetLayout vcfc_extract_workspace_layout(uint64_t n, uint64_t K) {
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
    L.seq_scratch = o; o = al(o + 8ull * VCFC_EXTRACT_SEQ_LANES * K);
    L.total = o;
    return L;
}

// blocks of the byte-serial kernels: a lane per record, VCFC_EXTRACT_SEQ_LANES at the most
static unsigned seq_blocks(uint64_t n) {
    const uint64_t want = (n + 63) / 64;
    return (unsigned)(want < VCFC_EXTRACT_SEQ_LANES / 64 ? want : VCFC_EXTRACT_SEQ_LANES / 64);
}

hipError_t vcfc_extract_plan(const VcfcExtractArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_ex_reset, dim3(1), dim3(64), 0, s, a.err, a.seq_count, a.n == 0 ? a.line_off : nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.n == 0) return e;
    const uint64_t per_block = EX_WAVES * (a.select ? SEL_R : 1);
    const dim3 grid((unsigned)((a.n + per_block - 1) / per_block)), block(64 * EX_WAVES);
    const bool small = a.K <= EX_TK_SMALL;
    if (a.select && small) hipLaunchKernelGGL((k_ex_plan<true, EX_TK_SMALL>), grid, block, 0, s, a);
    else if (a.select) hipLaunchKernelGGL((k_ex_plan<true, EX_TK>), grid, block, 0, s, a);
    else if (small) hipLaunchKernelGGL((k_ex_plan<false, EX_TK_SMALL>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_ex_plan<false, EX_TK>), grid, block, 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ex_seq, dim3(seq_blocks(a.n)), dim3(64), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return vcfc_scan_u32(a.line_size, a.n, a.partials, a.line_off, s);
}

hipError_t vcfc_extract_write(const VcfcExtractArgs &a, uint64_t first, uint64_t last, hipStream_t s) {
    if (last <= first) return hipSuccess;
    const uint64_t per_block = EX_WAVES * (a.select ? SEL_R : 1);
    const dim3 grid((unsigned)((last - first + per_block - 1) / per_block)), block(64 * EX_WAVES);
    const bool small = a.K <= EX_TK_SMALL;
    if (a.select && small) hipLaunchKernelGGL((k_ex_write<true, EX_TK_SMALL>), grid, block, 0, s, a, first, last);
    else if (a.select) hipLaunchKernelGGL((k_ex_write<true, EX_TK>), grid, block, 0, s, a, first, last);
    else if (small) hipLaunchKernelGGL((k_ex_write<false, EX_TK_SMALL>), grid, block, 0, s, a, first, last);
    else hipLaunchKernelGGL((k_ex_write<false, EX_TK>), grid, block, 0, s, a, first, last);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ex_wseq, dim3(seq_blocks(a.n)), dim3(64), 0, s, a, first, last);
    return hipGetLastError();
}
