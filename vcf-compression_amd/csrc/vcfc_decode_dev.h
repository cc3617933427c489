// vcfc_decode_dev.h -- device-side parsers of a .vcfc record shared by the
// decoder (vcfc_decode.hip), the sample-subset decoder (vcfc_subset.hip),
// genotype-counts (vcfc_counts.hip) and gap-analysis (vcfc_sparse_index.hip):
// the big-endian 30-bit header fields, the wave-parallel scan of a record's
// sample items, the record staged through LDS, the frame of a simple record
// (header bits, REQ, closing LF), the byte-serial walk of a regular record,
// and the records a wave takes in selected mode.  Everything here has
// internal linkage (anonymous namespace): each kernel file compiles its own
// copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vcfc_wave.h>   // angle brackets: tests/simt_emu shadows it

namespace {

constexpr uint32_t SB = 2048;              // sample bytes staged per piece (k_dec_write)
constexpr uint32_t SBUF = SB + 48;         // + look-ahead, 16-B alignment slack, last block's overhang

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// a header field (LEN, REQ length): 30 bits big-endian below the two flag bits
__device__ __forceinline__ uint32_t be30(const uint8_t *h) {
    return ((uint32_t)(h[0] & 0x3Fu) << 24) | ((uint32_t)h[1] << 16) | ((uint32_t)h[2] << 8) | h[3];
}

// bit i set <=> byte i of w is zero (exact)
// (the four flags gathered by one v_dot4_u32_u8, round 5: 6 VALU fewer than
// four shifts, masks and ors)
__device__ __forceinline__ uint32_t zero_bytes4(uint32_t w) {
    const uint32_t t = ~(((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w | 0x7F7F7F7Fu);
    return vw::dot4u(t >> 7, 0x08040201u, 0u);
}

// Record-relative positions below are 32-bit: a record is staged from the
// 16-byte block holding its first byte (rbase), and no record reaches 4 GiB.

// Wave-parallel scan of a record's sample items (see the header comment of
// vcfc_decode.hip), one window of 256 bytes per call: lane l holds the dword
// of bytes [b0 + 4l, b0 + 4l + 4) (b0 4-aligned); bytes outside [s0, b) are
// not part of the sample section (s0 may lie inside the first dword; byte s1
// is the record's LF).  Escape flag bytes (0xE1) mark the next 3 bytes as
// payload and the 4th as its terminator; those may spill into the next lane
// (DPP) or the next window (carry).  State carries across windows.
struct ItemState {
    uint32_t got = 0;
    uint32_t ecarry = 0;   // escape flags of the previous window's lane 63
    bool bad = false;
};
struct ItemLane {
    uint32_t start;    // bit j: byte j of the lane's dword starts an item
    uint32_t e1;       // bit j: byte j is an escape flag (0xE1)
    uint32_t gb[4];    // tokens before each byte's item
};

// bit j <- bit 8j + 7 of x (one flag per byte, as 0x80 in that byte)
__device__ __forceinline__ uint32_t msb4(uint32_t x) {
    return vw::dot4u((x >> 7) & 0x01010101u, 0x08040201u, 0u);
}
// bits [lo, hi) of a 4-bit mask (0 <= lo, hi <= 4)
__device__ __forceinline__ uint32_t bits4(uint32_t lo, uint32_t hi) {
    return ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// All four bytes of the lane at once (4-bit masks, one bit per byte): which
// bytes are in [s0, b), escape flags (0xE1), payload and terminator bytes,
// item starts and their token counts (a byte < 0x80 counts itself, a byte
// >= 0x80 its low 5 bits: 1 for 0xE1), and the checks of a simple record --
// payload bytes are < 0x80 and neither TAB nor LF, terminators are TAB, a
// start is not an escape code other than 0xE1, an escape's 3 bytes and
// terminator end before s1, and no item counts 0 tokens.
__device__ __forceinline__ ItemLane scan_window(uint32_t v4, uint32_t b0, uint32_t s0, uint32_t b, uint32_t s1,
                                                ItemState &st) {
    const uint32_t l = vw::lane_id();
    const uint32_t k0 = b0 + 4 * l;
    const uint32_t valid = bits4(s0 > k0 ? umin32(s0 - k0, 4u) : 0u, b > k0 ? umin32(b - k0, 4u) : 0u);
    const uint32_t tabM = zero_bytes4(v4 ^ 0x09090909u), lfM = zero_bytes4(v4 ^ 0x0A0A0A0Au);
    const uint32_t e1M = zero_bytes4(v4 ^ 0xE1E1E1E1u), escM = zero_bytes4((v4 & 0xE0E0E0E0u) ^ 0xE0E0E0E0u);
    const uint32_t hb = v4 & 0x80808080u;
    const uint32_t hi8 = (hb << 1) - (hb >> 7);                   // 0xFF in the bytes >= 0x80
    const uint32_t c8 = v4 & (~hi8 | 0x1F1F1F1Fu);                // each byte's token count
    const uint32_t e = valid & e1M;
    const uint32_t ep = vw::shr1(e, st.ecarry);     // escape flags of the previous lane
    st.ecarry = vw::readlane(e, 63);
    const uint32_t c = (e << 4) | ep;               // previous lane's bytes below this lane's
    const uint32_t P = ((c << 1) | (c << 2) | (c << 3)) >> 4 & 0xFu;   // payload bytes
    const uint32_t T = ep;                          // terminator bytes (4 after a flag)
    ItemLane r;
    r.start = valid & ~P & ~T;
    r.e1 = e1M;
    const int32_t lim = (int32_t)(s1 - k0) - 4;     // an escape at byte j needs j <= lim
    const uint32_t overM = lim >= 3 ? 0u : lim < 0 ? 0xFu : (0xFu << (lim + 1)) & 0xFu;
    const uint32_t bad = (P & ~T & (msb4(hb) | tabM | lfM)) | (T & ~tabM) |
                         (r.start & ((escM & ~e1M) | (e1M & overM) | zero_bytes4(c8)));
    st.bad = st.bad || vw::ballot((bad & valid) != 0) != 0;
    // start bits -> 0xFF bytes (bit j -> bit 8j by one 24-bit multiply), the
    // starts' counts, their sum and prefix sums by v_dot4_u32_u8
    const uint32_t s8 = vw::umul24(r.start, 0x00204081u) & 0x01010101u;
    const uint32_t cs = c8 & ((s8 << 8) - s8);      // counts of the starts
    const uint32_t sum = vw::dot4u(cs, 0x01010101u, 0u);
    const uint32_t inc = vw::scan_add(sum);
    const uint32_t base = st.got + (inc - sum);
    r.gb[0] = base;
    r.gb[1] = vw::dot4u(cs, 0x00000001u, base);
    r.gb[2] = vw::dot4u(cs, 0x00000101u, base);
    r.gb[3] = vw::dot4u(cs, 0x00010101u, base);
    st.got += vw::readlane(inc, 63);
    return r;
}

// A record staged through LDS in pieces of up to SB bytes (plus 8 bytes of
// look-ahead), loaded with 16-byte buffer loads: one load latency per piece
// instead of one per 64-byte window, and no global load between the
// writer's stores (vmcnt counts loads and stores together).  One buffer
// resource per record keeps offsets 32-bit for any input size; its range
// is rounded up to whole dwords (a dword only partly in range reads as 0; at
// most 3 bytes past the record are read, inside the input or its slack).
// Positions are relative to rbase = the record start rounded down to 16.
struct Staged {
    uint8_t *lds;
    vw::brsrc rsr;
    uint32_t re, cbase, cend;
    __device__ void init(uint8_t *l, const uint8_t *rec16, uint32_t rend) {
        lds = l;
        re = rend;
        rsr = vw::make_rsrc(rec16, (re + 3u) & ~3u);
        cbase = cend = 0;
    }
    // make [p, min(p + SB, re)) resident (wave-uniform p)
    __device__ void load(uint32_t p) {
        const uint32_t l = vw::lane_id();
        vw::wave_sync();   // everyone is done with the previous piece
        cbase = p & ~15u;
        cend = umin32(p + SB, re);
        const uint32_t lim = umin32(cend + 8, re);
        for (uint32_t o = 16u * l; cbase + o < lim; o += 1024)
            *reinterpret_cast<uint4 *>(lds + o) = vw::bload16(rsr, cbase + o);
        vw::wave_sync();
    }
    // window [k0, k0 + w) (clipped to re) resident
    __device__ __forceinline__ void need(uint32_t k0, uint32_t w = 64) {
        if (k0 < cbase || umin32(k0 + w, re) > cend) load(k0);
    }
    __device__ __forceinline__ uint32_t at(uint32_t k) const { return lds[k - cbase]; }
    // the dword at 4-aligned k (bytes past the staged data read as garbage)
    __device__ __forceinline__ uint32_t at4(uint32_t k) const { return *reinterpret_cast<const uint32_t *>(lds + (k - cbase)); }
};

// REQ bytes [r0, r0 + req): TAB count and the C-string length (first NUL).
__device__ __forceinline__ void scan_req(Staged &sg, uint32_t r0, uint32_t req, uint32_t *tabs, uint32_t *slen) {
    const uint32_t l = vw::lane_id();
    uint32_t t = 0, z = req;
    for (uint32_t b0 = 0; b0 < req; b0 += 64) {
        sg.need(r0 + b0);
        const uint32_t k = b0 + l;
        const uint32_t b = k < req ? sg.at(r0 + k) : 0xFFu;
        t += (uint32_t)vw::popc64(vw::ballot(b == '\t'));
        const uint64_t zm = vw::ballot(b == 0);
        if (zm && z == req) z = b0 + (uint32_t)__builtin_ctzll(zm);
    }
    *tabs = t;
    *slen = z;
}

// A record staged for a wave, positions relative to rbase: the record is
// [rs, re), its REQ bytes [rs + 8, rs + 8 + req), its sample items [s0(),
// s1()) and byte s1() its closing LF.  slen: REQ's C-string length (req where
// REQ holds no NUL).
struct RecFrame {
    uint32_t rs, re, req, slen;
    Staged sg;
    __device__ __forceinline__ uint32_t s0() const { return rs + 8 + req; }
    __device__ __forceinline__ uint32_t s1() const { return re - 1; }
};

// Stage the record in[rs_abs, re_abs) into sb and read its REQ length; no
// checks (the writers: the planner has validated the record; slen is not set).
__device__ __forceinline__ void frame_stage(RecFrame &f, uint8_t *sb, const uint8_t *in, uint64_t rs_abs, uint64_t re_abs) {
    const uint64_t rbase = rs_abs & ~15ull;
    f.rs = (uint32_t)(rs_abs - rbase);
    f.re = (uint32_t)(re_abs - rbase);
    f.sg.init(sb, in + rbase, f.re);
    f.sg.load(f.rs);
    f.req = be30(f.sg.lds + (f.rs + 4 - f.sg.cbase));
}

// The frame of a simple record: 10 <= length < 2^31, both header bytes' flag
// bits set, REQ not empty and ending before the record's last byte, exactly 9
// TABs in REQ, the last byte an LF.  (The last byte is touched after the REQ
// scan: a record longer than one staged piece is then loaded in order.)
__device__ __forceinline__ bool frame_open(RecFrame &f, uint8_t *sb, const uint8_t *in, uint64_t rs_abs, uint64_t re_abs) {
    if (re_abs - rs_abs < 10 || re_abs - rs_abs >= (1ull << 31)) return false;
    frame_stage(f, sb, in, rs_abs, re_abs);
    if ((f.sg.at(f.rs) >> 6) != 3u || (f.sg.at(f.rs + 4) >> 6) != 3u || f.req == 0 || 9 + (uint64_t)f.req >= f.re - f.rs)
        return false;
    uint32_t tabs;
    scan_req(f.sg, f.rs + 8, f.req, &tabs, &f.slen);
    f.sg.need(f.re - 1);
    return tabs == 9 && f.sg.at(f.re - 1) == '\n';
}

// Every window of the frame's sample items, up to the first that is not
// simple (bad): the record is simple when !bad && got == S.
__device__ __forceinline__ ItemState scan_items_plain(RecFrame &f) {
    const uint32_t l = vw::lane_id();
    const uint32_t s0 = f.s0(), s1 = f.s1();
    ItemState st;
    for (uint32_t cur = s0 & ~3u; cur < s1 && !st.bad; cur += 256) {
        f.sg.need(cur, 256 + 8);
        const uint32_t b = umin32(cur + 256, s1);
        (void)scan_window(f.sg.at4(cur + 4 * l), cur, s0, b, s1, st);
    }
    return st;
}

// The byte-serial walk of a regular record in[rs, re), one
// lane: false where the record is not regular.  REQCHK: REQ is checked too
// (no NUL, exactly 9 TABs).  token(got, src, len): column got holds the
// escaped token src[0, len); run(b, got, cnt): run byte b covers columns
// [got, got + cnt).
template <bool REQCHK, class FT, class FR>
__device__ __forceinline__ bool walk_regular(const uint8_t *in, uint64_t rs, uint64_t re, uint64_t S, FT token, FR run) {
    if (re - rs < 10 || re - rs >= (1ull << 31)) return false;
    const uint8_t *h = in + rs;
    if ((h[0] >> 6) != 3u || (h[4] >> 6) != 3u) return false;
    const uint32_t req = be30(h + 4);
    if (req == 0 || 9 + (uint64_t)req >= re - rs) return false;
    const uint64_t end = re - 1;   // the record's last byte: its LF
    if (in[end] != '\n') return false;
    if (REQCHK) {
        uint32_t tabs = 0;
        for (uint32_t k = 0; k < req; k++) {
            const uint8_t b = in[rs + 8 + k];
            if (b == 0) return false;
            tabs += b == '\t';
        }
        if (tabs != 9) return false;
    }
    uint64_t ip = rs + 8 + req, got = 0;
    while (got < S) {
        if (ip >= end) return false;
        const uint8_t b = in[ip++];
        if ((b & 0xE0u) == 0xE0u) {
            const uint32_t uc = b & 0x1Fu;
            if (got + uc > S) return false;
            for (uint32_t u = 0; u < uc; u++) {
                const uint64_t t0 = ip;
                while (ip < end && in[ip] != '\t' && in[ip] != '\n') ip++;
                // in[ip] is a TAB, or an LF: only the record's last token may end at the closing LF
                if (in[ip] == '\n' && (ip != end || u + 1 != uc || got + 1 != S)) return false;
                token(got, in + t0, (uint32_t)(ip - t0));
                got++;
                if (in[ip] == '\t') ip++;
            }
        } else {
            const uint32_t cnt = b < 0x80u ? b : (b & 0x1Fu);
            if (got + cnt > S) return false;
            run(b, got, cnt);
            got += cnt;
        }
    }
    return ip == end;   // the items end at the closing LF
}

// Selected mode (a select flag per record, the range query): a grid of about
// n / SEL_R waves; wave g of G takes records g, g + G, g + 2G, ... (SEL_R of
// them: lane l < SEL_R reads the flag of the l-th) and handles the selected
// ones, so an unselected record costs a flag read instead of a wave launch,
// and a contiguous selected range (a POS window) spreads over all waves.
// (The four selected kernels spell the dealing out, five lines each, around
// what each does with an unselected record and with its metadata.)
constexpr uint32_t SEL_R = 8;

}  // namespace
