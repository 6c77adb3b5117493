// Packed UNSTRUCTURED weights ("bm": bitmap): a linear under any bool mask -- what the 50 % unstructured Wanda prune, DSnoT, SparseGPT,
// the global pruners and every ECoFLaP allocation leave (wanda_pruner.py:330-337, the `mask` a prune puts on a module, :339) -- as
//     values [nnz + 16]      the kept weights, row after row in column order, then 16 zeros of tail
//     meta   [out, in / 8]   bit j of byte c is set exactly when column 8c + j is kept (the 4:8 byte of pack48.hip without its rule)
//     offs   [out, S] uint16 the number of kept columns of the row before column 32 s            S = ceil(in / 32)
//     rowptr [out + 1] int64 the index in values of the row's first kept weight; rowptr[out] == nnz
// so that chunk c of row n (step s = c / 4, quarter q = c % 4) starts at rowptr[n] + offs[n][s] + popcount(meta[n][4s .. 4s+q-1]):
// one dword of meta, one offs entry and one rowptr entry, no scan along the row.  The kept positions come from the MASK, not from
// the values: a kept +0 / -0 travels as it is, unpack(pack(W, mask)) == W . mask bit for bit and the mask is recovered.
// (16 d + 1.5) / 16 of the dense bytes at kept density d (+ 8 (out + 1) + 32): 9.5 / 16 at 50 %.  in <= 65536 keeps offs in 16 bits.
// One workgroup per row; a thread owns one chunk of 8 columns of a tile of 256 chunks and finds its place by a block-wide scan.
#include "common.hpp"
#include "wave_ops.hpp"

namespace vlmc {

// exclusive prefix of `cnt` over the 256 threads of the block and the block's total (all threads call it)
__device__ __forceinline__ uint32_t block256_excl_scan(const uint32_t cnt, uint32_t (&wsum)[4], uint32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan_u32_dpp(cnt);
    __syncthreads();                                                          // the previous tile's readers are done with wsum
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < 3; ++w) before += w < wave ? wsum[w] : 0u;
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return before + incl - cnt;
}

// rowptr[r + 1] = kept columns of row r
__global__ __launch_bounds__(256) void packbm_count_kernel(const uint8_t *__restrict__ mask, int64_t ldm, int64_t in_f, int64_t *__restrict__ rowptr) {
    __shared__ uint32_t wsum[4];
    const uint8_t *m = mask + int64_t(blockIdx.x) * ldm;
    uint32_t n = 0;
    for (int64_t i = threadIdx.x; i < in_f; i += 256) n += m[i] != 0;
    n = wave_sum_u32_dpp(n);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) rowptr[int64_t(blockIdx.x) + 1] = int64_t(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

// rowptr[0] = 0, rowptr[r + 1] = the counts' inclusive prefix sum: one block, a contiguous run of rows per thread
__global__ __launch_bounds__(1024) void packbm_scan_kernel(int64_t *__restrict__ rowptr, int64_t out_f) {
    __shared__ int64_t part[1024];
    const int64_t per = (out_f + 1023) / 1024, lo = min(int64_t(threadIdx.x) * per, out_f), hi = min(lo + per, out_f);
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += rowptr[i + 1];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int t = 0; t < 1024; ++t) {
            const int64_t p = part[t];
            part[t] = run;
            run += p;
        }
        rowptr[0] = 0;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) {
        run += rowptr[i + 1];
        rowptr[i + 1] = run;
    }
}

__global__ __launch_bounds__(256) void packbm_kernel(const uint16_t *__restrict__ W, int64_t ldw, const uint8_t *__restrict__ mask, int64_t ldm,
                                                     int64_t out_f, int64_t in_f, const int64_t *__restrict__ rowptr, int64_t nnz,
                                                     uint16_t *__restrict__ values, uint8_t *__restrict__ meta, uint16_t *__restrict__ offs) {
    __shared__ uint32_t wsum[4];
    const int64_t r = blockIdx.x, chunks = in_f / 8, S = (chunks + 3) / 4, rp = rowptr[r];
    uint32_t base = 0;
    for (int64_t c0 = 0; c0 < chunks; c0 += 256) {
        const int64_t c = c0 + threadIdx.x;
        const bool in = c < chunks;
        uint16_t w[8];
        unsigned bits = 0;
        if (in) {
            const uint16_t *wp = W + r * ldw + c * 8;
            const uint8_t *mp = mask + r * ldm + c * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = wp[j], bits |= unsigned(mp[j] != 0) << j;
        }
        uint32_t total;
        const uint32_t first = base + block256_excl_scan(uint32_t(__popc(bits)), wsum, total);
        if (in) {
            meta[r * chunks + c] = uint8_t(bits);
            if ((c & 3) == 0) offs[r * S + (c >> 2)] = uint16_t(first);
            int64_t o = rp + first;                                           // (rowptr is the caller's: never write outside [0, nnz))
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((bits >> j) & 1u) {
                    if (o >= 0 && o < nnz) values[o] = w[j];
                    ++o;
                }
        }
        base += total;
    }
    if (r == out_f - 1 && threadIdx.x < 16) values[nnz + threadIdx.x] = 0;   // the tail the forward's 16-byte fetches may touch
}

// The chunk's first value is looked up the way the forward does it (rowptr + offs + the step's popcount so far), CLAMPED to
// [0, nnz]: whatever the metadata holds, nothing outside values[0, nnz + 16) is read.  The running popcount of the bitmap is kept
// beside it, and *bad counts every step whose offs and every row whose rowptr pair disagree with it (and rowptr[0] != 0,
// rowptr[out] != nnz).
__global__ __launch_bounds__(256) void unpackbm_kernel(const uint16_t *__restrict__ values, const uint8_t *__restrict__ meta,
                                                       const uint16_t *__restrict__ offs, const int64_t *__restrict__ rowptr, int64_t nnz,
                                                       int64_t out_f, int64_t in_f, uint16_t *__restrict__ W, int64_t ldw, uint8_t *__restrict__ mask,
                                                       int64_t ldm, unsigned int *__restrict__ bad) {
    __shared__ uint32_t wsum[4];
    const int64_t r = blockIdx.x, chunks = in_f / 8, S = (chunks + 3) / 4, rp = rowptr[r];
    uint32_t base = 0;
    for (int64_t c0 = 0; c0 < chunks; c0 += 256) {
        const int64_t c = c0 + threadIdx.x;
        const bool in = c < chunks;
        const unsigned bits = in ? meta[r * chunks + c] : 0u;
        uint32_t total;
        const uint32_t first = base + block256_excl_scan(uint32_t(__popc(bits)), wsum, total);
        if (in) {
            const int64_t s = c >> 2;
            const unsigned off = offs[r * S + s];
            if ((c & 3) == 0 && off != first) atomicAdd(bad, 1u);
            unsigned before = 0;
            for (int64_t p = 4 * s; p < c; ++p) before += unsigned(__popc(unsigned(meta[r * chunks + p])));
            int64_t i = rp + int64_t(off) + int64_t(before);
            i = i < 0 ? 0 : (i > nnz ? nnz : i);
            uint16_t *o = W + r * ldw + c * 8;
            uint8_t *mo = mask ? mask + r * ldm + c * 8 : nullptr;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool k = (bits >> j) & 1u;
                w[j >> 1] |= uint32_t(k ? values[i] : uint16_t(0)) << (16 * (j & 1));
                i += k;
                if (mo) mo[j] = uint8_t(k);
            }
            if ((reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
                *reinterpret_cast<u32x4_t *>(o) = u32x4_t{w[0], w[1], w[2], w[3]};
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = uint16_t(w[j >> 1] >> (16 * (j & 1)));
            }
        }
        base += total;
    }
    if (threadIdx.x == 0) {
        unsigned wrong = rowptr[r + 1] - rp != int64_t(base);
        wrong += r == 0 && rp != 0;
        wrong += r == out_f - 1 && rowptr[out_f] != nnz;
        if (wrong) atomicAdd(bad, wrong);
    }
}

}  // namespace vlmc

using namespace vlmc;

#define VLMC_BM_SHAPE(fn)                                                                                                                    \
    VLMC_REQUIRE(out_features > 0 && in_features > 0 && in_features % 8 == 0 && in_features <= 65536 && out_features < (int64_t(1) << 31), \
                 fn ": in_features must be a positive multiple of 8, at most 65536")

extern "C" int vlmc_pack_bm_rows(const uint8_t *mask, int64_t ldm, int64_t out_features, int64_t in_features, int64_t *rowptr, void *stream) {
    VLMC_REQUIRE(mask && rowptr, "vlmc_pack_bm_rows: null pointer");
    VLMC_BM_SHAPE("vlmc_pack_bm_rows");
    VLMC_REQUIRE(ldm >= in_features, "vlmc_pack_bm_rows: bad shape");
    hipLaunchKernelGGL(packbm_count_kernel, dim3(unsigned(out_features)), dim3(256), 0, as_stream(stream), mask, ldm, in_features, rowptr);
    hipLaunchKernelGGL(packbm_scan_kernel, dim3(1), dim3(1024), 0, as_stream(stream), rowptr, out_features);
    VLMC_HIP_CHECK_LAUNCH("vlmc_pack_bm_rows");
    return VLMC_OK;
}

extern "C" int vlmc_pack_bm(const void *W, int dtype, int64_t out_features, int64_t in_features, int64_t ldw, const uint8_t *mask, int64_t ldm,
                            const int64_t *rowptr, int64_t nnz, void *values, uint8_t *meta, uint16_t *offs, void *stream) {
    VLMC_REQUIRE(dtype == VLMC_F16 || dtype == VLMC_BF16, "vlmc_pack_bm: dtype must be VLMC_F16 or VLMC_BF16");
    VLMC_REQUIRE(W && mask && rowptr && values && meta && offs, "vlmc_pack_bm: null pointer");
    VLMC_BM_SHAPE("vlmc_pack_bm");
    VLMC_REQUIRE(ldw >= in_features && ldm >= in_features && nnz >= 0 && nnz <= out_features * in_features, "vlmc_pack_bm: bad shape");
    hipLaunchKernelGGL(packbm_kernel, dim3(unsigned(out_features)), dim3(256), 0, as_stream(stream), static_cast<const uint16_t *>(W), ldw, mask, ldm,
                       out_features, in_features, rowptr, nnz, static_cast<uint16_t *>(values), meta, offs);
    VLMC_HIP_CHECK_LAUNCH("vlmc_pack_bm");
    return VLMC_OK;
}

extern "C" int vlmc_unpack_bm(const void *values, const uint8_t *meta, const uint16_t *offs, const int64_t *rowptr, int64_t nnz, int dtype,
                              int64_t out_features, int64_t in_features, void *W, int64_t ldw, uint8_t *mask, int64_t ldm, unsigned int *bad,
                              void *stream) {
    VLMC_REQUIRE(dtype == VLMC_F16 || dtype == VLMC_BF16, "vlmc_unpack_bm: dtype must be VLMC_F16 or VLMC_BF16");
    VLMC_REQUIRE(W && values && meta && offs && rowptr && bad, "vlmc_unpack_bm: null pointer");
    VLMC_BM_SHAPE("vlmc_unpack_bm");
    VLMC_REQUIRE(ldw >= in_features && (!mask || ldm >= in_features) && nnz >= 0 && nnz <= out_features * in_features, "vlmc_unpack_bm: bad shape");
    hipLaunchKernelGGL(unpackbm_kernel, dim3(unsigned(out_features)), dim3(256), 0, as_stream(stream), static_cast<const uint16_t *>(values), meta,
                       offs, rowptr, nnz, out_features, in_features, static_cast<uint16_t *>(W), ldw, mask, ldm, bad);
    VLMC_HIP_CHECK_LAUNCH("vlmc_unpack_bm");
    return VLMC_OK;
}
