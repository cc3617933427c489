// wave_probe.hip -- TEST INFRASTRUCTURE ONLY: one tiny kernel per family of
// wave primitives in vcfc_wave.h, so that the product header (csrc/) and its
// emulated twin (tests/simt_emu/) can both be held to a plain statement of
// each operation (tests/test_wave_twin.py on the CPU, tests/test_gpu_wave.py
// on the GPU).  The header comes in angle brackets: this file compiles
// against either one, as the kernel sources do.
//
// Every kernel runs one block of 256 threads (4 waves).  Thread t = 64 w + l
// reads its inputs at [t] and writes result k at out[256 k + t].
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vcfc_wave.h>

namespace {

constexpr uint32_t NT = 256;

// lane identity and cross-lane moves: 20 results
__global__ __launch_bounds__(256) void k_lanes(const uint32_t *a, const uint32_t *b, uint32_t *out) {
    const uint32_t t = threadIdx.x;
    const uint32_t x = a[t], y = b[t];
    uint32_t k = 0;
    auto put = [&](uint32_t v) { out[NT * k++ + t] = v; };
    put(vw::lane_id());
    const uint64_t bal = vw::ballot((x & 1u) != 0);
    put((uint32_t)bal);
    put((uint32_t)(bal >> 32));
    const uint64_t lt = vw::lanemask_lt();
    put((uint32_t)lt);
    put((uint32_t)(lt >> 32));
    put(vw::readfirst(x));
    put(vw::readlane(x, 0));
    put(vw::readlane(x, 15));
    put(vw::readlane(x, 16));
    put(vw::readlane(x, 31));
    put(vw::readlane(x, 32));
    put(vw::readlane(x, 47));
    put(vw::readlane(x, 48));
    put(vw::readlane(x, 63));
    put(vw::readlane(x, vw::readfirst(y) & 63u));   // a lane index the compiler does not know
    put(vw::shr1(x, y));
    put(vw::shr1z(x));
    put(vw::shl1(x, y));
    put(vw::row_shl1(x));
    put(vw::shfl(x, y & 63u));
}

// the scans, each straight after a VALU producer of its operand
// (v = a * b + c), twice back to back, and again on a fresh VALU result:
// nothing but the scan's own leading wait states covers the hazard; and a DPP
// move straight off a scan's result, as the decoder's tiles take it.  11 results
__global__ __launch_bounds__(256) void k_scans(const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out) {
    const uint32_t t = threadIdx.x;
    const uint32_t x = a[t], y = b[t], z = c[t];
    const uint32_t s1 = vw::scan_add(x * y + z);
    const uint32_t s2 = vw::scan_add(s1);
    const uint32_t s3 = vw::scan_add(s2 ^ x);
    const uint32_t n1 = vw::scan_last_nz(x * y + z);
    const uint32_t n2 = vw::scan_last_nz(n1);
    const uint32_t n3 = vw::scan_last_nz(n1 ^ (x * y + z));   // (zero where the lane's own value came through)
    const uint32_t m1 = vw::scan_max(x * y + z);
    const uint32_t m2 = vw::scan_max(m1);
    const uint32_t m3 = vw::scan_max(m1 - (x * y + z));
    const uint32_t d1 = vw::shr1z(vw::scan_last_nz(x + y));
    const uint32_t d2 = vw::shr1(vw::scan_add(x + y), z);
    const uint32_t r[11] = {s1, s2, s3, n1, n2, n3, m1, m2, m3, d1, d2};
    for (uint32_t k = 0; k < 11; k++) out[NT * k + t] = r[k];
}

// in-lane arithmetic: 15 results.  c carries the selectors and shift counts.
__global__ __launch_bounds__(256) void k_bits(const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *sel,
                                              uint32_t *out) {
    const uint32_t t = threadIdx.x;
    const uint32_t x = a[t], y = b[t], z = c[t];
    uint32_t k = 0;
    auto put = [&](uint32_t v) { out[NT * k++ + t] = v; };
    put(vw::perm(x, y, sel[t]));          // selector bytes 0..7 and 0x0C: the only ones the kernels use
    put(vw::alignbit(x, y, z & 31u));
    put(vw::alignbyte(x, y, z & 3u));
    put((uint32_t)vw::mad24((int32_t)x, (int32_t)y, (int32_t)z));
    put(vw::umul24(x, y));
    put((uint32_t)vw::mulsel((int32_t)x, (int32_t)y));
    put(vw::dot4u(x, y, z));
    put(vw::bfi(z, x, y));
    put((uint32_t)vw::sbit(x, z & 31u));
    put(vw::mulhi(x, y));
    put(x ? vw::ffbl(x) : 0xFFu);         // (unspecified for 0)
    const uint64_t m = ((uint64_t)x << 32) | y;
    put((uint32_t)vw::popc64(m));
    put(m ? (uint32_t)vw::hibit64(m) : 0xFFu);
    put(vw::umax(x, y));
    put(vw::alignbyte(y, x, (z >> 8) % 3u + 1u));   // the decoder's use: shifts 1..3
}

// LDS byte stores: each lane owns 32 bytes of its wave's buffer, preset to
// 0xEE.  lds_sel's address is lds + dm + f * x with f = a & 1, x = b % 5 and
// dm = 32 l + {1, 9, 17} + c % 3, so stores land at odd and even addresses
// inside the lane's bytes: two byte stores from the low half of v, two from
// the high half, one unaligned dword.  8 results: the lane's 32 bytes.
__global__ __launch_bounds__(256) void k_lds(const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *v,
                                             uint32_t *out) {
    __shared__ __attribute__((aligned(16))) uint8_t buf[4 * 64 * 32];
    const uint32_t t = threadIdx.x, l = vw::lane_id();
    uint8_t *wb = buf + (t >> 6) * (64 * 32);
    for (uint32_t q = 0; q < 8; q++) *reinterpret_cast<uint32_t *>(wb + 32 * l + 4 * q) = 0xEEEEEEEEu;
    vw::wave_sync();
    const int32_t f = (int32_t)(a[t] & 1u), x = (int32_t)(b[t] % 5u), d = (int32_t)(c[t] % 3u);
    const uint32_t val = v[t];
    const vw::ldsp p0 = vw::lds_sel(wb, f, x, (int32_t)(32 * l) + 1 + d);
    vw::lds_st8<0, false>(p0, val);
    vw::lds_st8<1, true>(p0, val);
    const vw::ldsp p1 = vw::lds_sel(wb, f, x, (int32_t)(32 * l) + 9 + d);
    vw::lds_st8<0, true>(p1, val);
    vw::lds_st8<1, false>(p1, val);
    const vw::ldsp p2 = vw::lds_sel(wb, f, x, (int32_t)(32 * l) + 17 + d);
    vw::lds_st32(p2, val);
    vw::wave_sync();
    for (uint32_t q = 0; q < 8; q++) out[NT * q + t] = *reinterpret_cast<const uint32_t *>(wb + 32 * l + 4 * q);
}

// 16-byte global accesses at every byte alignment: thread t loads the 16
// bytes at src + 32 t + t % 16 (4 results) and stores them at the same offset
// of dst (plain) and dst_nt (non-temporal); src, dst, dst_nt hold 32 * 256
// bytes, and the test looks at every byte of the two.
__global__ __launch_bounds__(256) void k_global(const uint8_t *src, uint8_t *dst, uint8_t *dst_nt, uint32_t *out) {
    const uint32_t t = threadIdx.x;
    const uint32_t off = 32 * t + (t & 15u);
    const uint4 v = vw::uload16(src + off);
    out[t] = v.x;
    out[NT + t] = v.y;
    out[2 * NT + t] = v.z;
    out[3 * NT + t] = v.w;
    vw::gstore16(dst, off, v);
    vw::gstore16_nt(dst_nt, off, make_uint4(~v.x, ~v.y, ~v.z, ~v.w));
}

// Raw-buffer loads over [src, src + bytes): thread t loads 16 bytes and 4
// bytes at offset off[t], with the default and the non-temporal cache policy.
// 10 results.  src holds non-zero bytes well past `bytes`.
__global__ __launch_bounds__(256) void k_buffer(const uint8_t *src, uint32_t bytes, const uint32_t *off, uint32_t *out) {
    const uint32_t t = threadIdx.x;
    const vw::brsrc r = vw::make_rsrc(src, bytes);
    const uint32_t o = off[t];
    const uint4 v = vw::bload16(r, o);
    const uint4 n = vw::bload16(r, o, 2);
    out[t] = v.x;
    out[NT + t] = v.y;
    out[2 * NT + t] = v.z;
    out[3 * NT + t] = v.w;
    out[4 * NT + t] = vw::bload4(r, o);
    out[5 * NT + t] = n.x;
    out[6 * NT + t] = n.y;
    out[7 * NT + t] = n.z;
    out[8 * NT + t] = n.w;
    out[9 * NT + t] = vw::bload4(r, o, 2);
}

}  // namespace

extern "C" {
int wave_probe_lanes(const uint32_t *a, const uint32_t *b, uint32_t *out, hipStream_t s) {
    hipLaunchKernelGGL(k_lanes, dim3(1), dim3(256), 0, s, a, b, out);
    return (int)hipGetLastError();
}
int wave_probe_scans(const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out, hipStream_t s) {
    hipLaunchKernelGGL(k_scans, dim3(1), dim3(256), 0, s, a, b, c, out);
    return (int)hipGetLastError();
}
int wave_probe_bits(const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *sel, uint32_t *out,
                    hipStream_t s) {
    hipLaunchKernelGGL(k_bits, dim3(1), dim3(256), 0, s, a, b, c, sel, out);
    return (int)hipGetLastError();
}
int wave_probe_lds(const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *v, uint32_t *out,
                   hipStream_t s) {
    hipLaunchKernelGGL(k_lds, dim3(1), dim3(256), 0, s, a, b, c, v, out);
    return (int)hipGetLastError();
}
int wave_probe_global(const uint8_t *src, uint8_t *dst, uint8_t *dst_nt, uint32_t *out, hipStream_t s) {
    hipLaunchKernelGGL(k_global, dim3(1), dim3(256), 0, s, src, dst, dst_nt, out);
    return (int)hipGetLastError();
}
int wave_probe_buffer(const uint8_t *src, uint32_t bytes, const uint32_t *off, uint32_t *out, hipStream_t s) {
    hipLaunchKernelGGL(k_buffer, dim3(1), dim3(256), 0, s, src, bytes, off, out);
    return (int)hipGetLastError();
}
}
