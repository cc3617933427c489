// vcfc_bed_planes.h -- 32 samples of a .bed row as one word of each of the three
// bit planes H (g = 1), B (g = 2), V (called); shared by ld-window
// (vcfc_ld.hip, sample-major words of a row) and kinship (vcfc_kin.hip, which
// transposes them).  A .bed code is 2 bits a sample: 11 g = 0, 10 g = 1,
// 00 g = 2, 01 missing.
#pragma once
#include <stdint.h>
#include <vcfc_wave.h>   // angle brackets: tests/simt_emu shadows it

namespace vcfc_bed {

// bits 0, 2, 4, ... of x as the low 32 bits
__device__ __forceinline__ uint32_t even_bits(uint64_t x) {
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    return (uint32_t)(x | (x >> 16));
}

// Samples [32 w, 32 w + 32) of a row of rb bytes and S samples (w < ceil(S /
// 32)), p = the row + 8 w, any alignment: the 8 row bytes come out of the (at
// most three) aligned words that hold them; only words that hold a byte of the
// row are loaded.  Columns >= S are 0 in all three planes.
__device__ __forceinline__ void word_planes(const uint8_t *p, uint32_t w, uint32_t S, uint32_t rb, uint32_t &H, uint32_t &B,
                                            uint32_t &V) {
    const uint32_t nb = 8u < rb - 8u * w ? 8u : rb - 8u * w;   // the row's bytes behind p
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - sh);
    const uint32_t d0 = q[0];
    const uint32_t d1 = sh + nb > 4u ? q[1] : 0u;
    const uint32_t d2 = sh + nb > 8u ? q[2] : 0u;
    uint64_t x = (uint64_t)vw::alignbyte(d1, d0, sh) | ((uint64_t)vw::alignbyte(d2, d1, sh) << 32);
    if (nb < 8u) x &= (1ull << (8u * nb)) - 1ull;
    const uint32_t lo = even_bits(x), hi = even_bits(x >> 1);
    const uint32_t left = S - 32u * w;                     // columns of the word that exist
    const uint32_t m = left >= 32u ? ~0u : (1u << left) - 1u;
    H = hi & ~lo & m;
    B = ~hi & ~lo & m;
    V = (hi | ~lo) & m;
}

}  // namespace vcfc_bed
