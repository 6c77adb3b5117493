// One pack chunk of the n:m formats (8 bytes of values + 1 byte of meta per 8 input columns: pack24.hip, pack48.hip) -> its 8 weights
// in registers.  Shared by linear24.hip (the A fragment of the carried-chain kernel) and gemm_nt.hip (the P operand of the tiled
// kernel on its way into LDS).
#pragma once
#include "common.hpp"

namespace vlmc {

// 2:4.  Per group of four: code = i0 | i1 << 2 (i0 < i1), the two kept values go to positions i0 and i1, the others are +0.  Two
// 2-bit indices cannot address outside their group.
__device__ __forceinline__ u32x4_t expand24(const u32x2_t v, const uint32_t code) {
    u32x4_t w;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const uint32_t c = code >> (4 * g);
        const uint64_t lo = uint64_t(v[g] & 0xffffu) << (16 * (c & 3u)), hi = uint64_t(v[g] >> 16) << (16 * ((c >> 2) & 3u));
        const uint64_t grp = lo | hi;
        w[2 * g] = uint32_t(grp), w[2 * g + 1] = uint32_t(grp >> 32);
    }
    return w;
}

// Selector dword d (positions 2d, 2d + 1) of bitmap byte e for v_perm_b32 over the value halfwords base .. base + 3: bit p of e
// says that position p holds the next value, value r = popcount of the bits below p.  A position whose value is one of the four
// gets that halfword's two bytes, every other position 0x0c0c (v_perm_b32's constant 0x00).
__device__ __forceinline__ uint32_t perm_selector(uint32_t e, uint32_t d, uint32_t base) {
    uint32_t s = 0x0c0c0c0cu;
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
        const uint32_t p = 2 * d + h, r = uint32_t(__popc(e & ((1u << p) - 1u))) - base;   // position p takes value base + r
        if (((e >> p) & 1u) && r < 4) s = (s & ~(0xffffu << (16 * h))) | ((2 * r) | (2 * r + 1) << 8) << (16 * h);
    }
    return s;
}

// The selector table of values base .. base + 3: byte -> four selector dwords, 256 x 16 B = 4 KiB of LDS at `table`, filled by a
// workgroup of NT threads (1024: one thread per dword; fewer: a loop).  The caller's barrier publishes it.
template <int NT, uint32_t BASE> __device__ __forceinline__ void fill_perm_table(uint32_t *table, int tid) {
    if constexpr (NT == 1024) {
        table[tid] = perm_selector(uint32_t(tid) >> 2, uint32_t(tid) & 3u, BASE);
    } else {
        static_assert(1024 % NT == 0, "whole rounds");
#pragma unroll
        for (int i = tid; i < 1024; i += NT) table[i] = perm_selector(uint32_t(i) >> 2, uint32_t(i) & 3u, BASE);
    }
}

// 4:8 (and the first four values of a bm chunk): the chunk's 8 bytes are exactly the sources of v_perm_b32 ({v[1], v[0]}: selector
// s picks byte s of the chunk, 0x0c gives 0x00), so each output dword is one perm whose selector comes from the table.  A selector
// never names anything but a byte of the chunk or zero, and the table is indexed by a byte: whatever the metadata holds, nothing
// outside the chunk is read.
__device__ __forceinline__ u32x4_t expand48(const u32x2_t v, const u32x4_t s) {
    u32x4_t w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = __builtin_amdgcn_perm(v[1], v[0], s[j]);
    return w;
}

}  // namespace vlmc
