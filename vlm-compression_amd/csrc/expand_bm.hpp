// One pack chunk of the bitmap format (packbm.hip: values [nnz + 16], meta [N, K / 8], offs [N, ceil(K / 32)], rowptr [N + 1]) -> its 8
// weights in registers.  Shared by linear24.hip (ExpandBM: the A fragment of the carried-chain kernel) and gemm_nt.hip (PackedBM: the P
// operand of the tiled kernel on its way into LDS).
//
// The byte means what the 4:8 byte means, with 0 to 8 bits set.  The chunk's values are the 0 to 8 halfwords from index
//     i = clamp(rowptr[n] + offs[n][s] + popcount(the step's meta bytes before this quarter), 0, nnz)
// of `values`, fetched as the FIVE ALIGNED dwords from i >> 1 (one 16-byte load that needs 4-byte alignment only, one dword) and
// shifted down by the odd halfword with v_alignbyte_b32 -- halfwords i & ~1 .. (i & ~1) + 9 <= nnz + 9, inside the 16 of tail
// whatever the metadata holds.  The step's four meta bytes sit at byte wrow * K / 8 + 4 s of `meta`, at any alignment: the two
// aligned dwords round it, the second clamped to the last dword that holds a byte of meta (its bytes are then other chunks' or
// none's: only the bytes of chunks < K / 8 of this row are ever used).
// Expansion: value r of the chunk is halfword r of the four shifted dwords {v0 .. v3}; output dword j is
// perm({v1, v0}, A[byte][j]) | perm({v3, v2}, B[byte][j]) with A the selectors of values 0..3 (the 4:8 table) and B those of values
// 4..7, 0x0c for "not from this pair": 8 KiB of LDS.
// The address of the values depends on meta and offs, so a kernel fetches those one round further ahead than the values (`prime`).
#pragma once
#include "common.hpp"
#include "expand_nm.hpp"

namespace vlmc {

typedef uint32_t u32x4_a4_t __attribute__((ext_vector_type(4), aligned(4)));

// both selector tables, [0, 256): A, [256, 512): B, filled by a workgroup of NT threads; the caller's barrier publishes them
template <int NT> __device__ __forceinline__ void fill_bm_tables(u32x4_t *table, int tid) {
    fill_perm_table<NT, 0>(reinterpret_cast<uint32_t *>(table), tid);
    fill_perm_table<NT, 4>(reinterpret_cast<uint32_t *>(table) + 1024, tid);
}

// what a thread holds of D chunks between the loads and the expansion
template <int D> struct BMRegs {
    u32x4_t v[D];                          // the aligned dwords 0..3 from i >> 1, v4: the fifth
    uint32_t v4[D], code[D];               // code: the chunk's byte | (i & 1) << 8
    uint32_t mlo[D], mhi[D], off[D];       // primed: the two aligned dwords round the step's meta bytes, offs[n][s]
};

// where a thread's chunks of ONE weight row are: every chunk it asks for has the same quarter (chunk % 4) of its step
struct BMRow {
    const u32x4_t *sel;                        // fill_bm_tables' tables
    const uint32_t *val32, *meta32;
    const uint16_t *orow;
    int64_t rp, nnz, mbyte, last_dw;
    int chunks;
    uint32_t q8;
    // wrow < N: the row;   quarter: this thread's chunk % 4
    __device__ __forceinline__ void row(const uint16_t *values, const uint8_t *meta, const uint16_t *offs, const int64_t *rowptr, int64_t nnz_, int N,
                                        int K, int wrow, int quarter) {
        chunks = K >> 3;
        val32 = reinterpret_cast<const uint32_t *>(values), meta32 = reinterpret_cast<const uint32_t *>(meta);
        orow = offs + int64_t(wrow) * ((chunks + 3) >> 2);
        rp = rowptr[wrow], nnz = nnz_;
        mbyte = int64_t(wrow) * chunks, last_dw = (int64_t(N) * chunks - 1) >> 2;
        q8 = 8u * uint32_t(quarter);
    }
    // issue the metadata loads of chunk cc (< K / 8) into slot d
    template <int D> __device__ __forceinline__ void prime(BMRegs<D> &R, int d, int cc) const {
        const int s = cc >> 2;
        const int64_t w = (mbyte + 4 * s) >> 2;                       // (chunk 4 s of this row exists: w <= last_dw)
        R.mlo[d] = meta32[w];
        R.mhi[d] = meta32[min(w + 1, last_dw)];
        R.off[d] = orow[s];
    }
    // from the primed metadata of chunk cc in slot d: its code and the loads of its five dwords; then prime chunk `ahead` there
    template <int D> __device__ __forceinline__ void load(BMRegs<D> &R, int d, int cc, int ahead) const {
        const int s = cc >> 2;                                        // (a clamped chunk keeps this thread's quarter: any valid address)
        const uint32_t m = __builtin_amdgcn_alignbyte(R.mhi[d], R.mlo[d], uint32_t(mbyte + 4 * s) & 3u);
        const uint32_t before = uint32_t(__popc(m & ((1u << q8) - 1u)));
        const int64_t i = max(min(rp + int64_t(R.off[d] + before), nnz), int64_t(0));
        R.code[d] = ((m >> q8) & 0xffu) | uint32_t(i & 1) << 8;
        const uint32_t *p = val32 + (i >> 1);
        R.v[d] = *reinterpret_cast<const u32x4_a4_t *>(p);
        R.v4[d] = p[4];
        prime(R, d, ahead);
    }
    // slot d's 8 weights
    template <int D> __device__ __forceinline__ u32x4_t expand(const BMRegs<D> &R, int d) const {
        const uint32_t code = R.code[d], sh = (code >> 8) << 1;       // 0 or 2 bytes
        const u32x4_t r = R.v[d];
        const uint32_t v0 = __builtin_amdgcn_alignbyte(r[1], r[0], sh), v1 = __builtin_amdgcn_alignbyte(r[2], r[1], sh),
                       v2 = __builtin_amdgcn_alignbyte(r[3], r[2], sh), v3 = __builtin_amdgcn_alignbyte(R.v4[d], r[3], sh);
        const u32x4_t sa = sel[code & 0xffu], sb = sel[256u + (code & 0xffu)];
        u32x4_t w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = __builtin_amdgcn_perm(v1, v0, sa[j]) | __builtin_amdgcn_perm(v3, v2, sb[j]);
        return w;
    }
};

}  // namespace vlmc
