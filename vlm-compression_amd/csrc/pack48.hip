// Packed 4:8 weights: a linear whose mask keeps exactly four of every eight consecutive input columns (the n:m rule of
// wanda_pruner.py:326-329 at prune_n = 4, prune_m = 8) stored as
//     values [out, in / 2]   the kept weights in column order
//     meta   [out, in / 8]   one byte per group of eight: bit j is set exactly when column 8c + j is kept (popcount 4)
// 9 / 16 of the dense bytes for 16-bit weights, as the 2:4 format of pack24.hip, and the same chunk: 8 bytes of values and one byte
// of meta per 8 input columns.  The kept positions come from the MASK, not from the values: a kept weight that happens to be zero
// stays a kept zero, so unpack(pack(W, mask)) == W . mask bit for bit and the mask itself is recovered.  Every 2:4 mask is also a
// 4:8 mask and packs here too; the selector form of pack24.hip is what a caller who wants it asks for first.
// HBM-bound, one pass: a lane owns 8 columns (16 B of weights, 8 mask bytes) -> 8 B of values + 1 byte of meta.
#include "common.hpp"

namespace vlmc {

__global__ __launch_bounds__(256) void pack48_kernel(const uint16_t *__restrict__ W, int64_t ldw, const uint8_t *__restrict__ mask, int64_t ldm,
                                                     int64_t out_f, int64_t in_f, uint16_t *__restrict__ values, uint8_t *__restrict__ meta,
                                                     unsigned int *__restrict__ bad) {
    const int64_t chunks = in_f / 8, i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= out_f * chunks) return;
    const int64_t r = i / chunks, c = i - r * chunks;
    const uint16_t *w = W + r * ldw + c * 8;
    const uint8_t *m = mask + r * ldm + c * 8;
    uint16_t v[4] = {0, 0, 0, 0};
    unsigned bits = 0, n = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool k = m[j] != 0;
        const uint16_t wj = w[j];
#pragma unroll
        for (int s = 0; s < 4; ++s) v[s] = (k && n == unsigned(s)) ? wj : v[s];   // the first four kept, in column order
        bits |= unsigned(k) << j;
        n += k;
    }
    if (n != 4) atomicAdd(bad, 1u);
    uint16_t *o = values + r * (in_f / 2) + c * 4;
    o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3];
    meta[r * chunks + c] = uint8_t(bits);
}

__global__ __launch_bounds__(256) void unpack48_kernel(const uint16_t *__restrict__ values, const uint8_t *__restrict__ meta, int64_t out_f,
                                                       int64_t in_f, uint16_t *__restrict__ W, int64_t ldw, uint8_t *__restrict__ mask, int64_t ldm,
                                                       unsigned int *__restrict__ bad) {
    const int64_t chunks = in_f / 8, i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= out_f * chunks) return;
    const int64_t r = i / chunks, c = i - r * chunks;
    const uint16_t *vp = values + r * (in_f / 2) + c * 4;
    const uint16_t v[4] = {vp[0], vp[1], vp[2], vp[3]};
    const unsigned bits = meta[r * chunks + c];
    if (__popc(bits) != 4) atomicAdd(bad, 1u);                                // (never written by pack48_kernel)
    uint16_t *o = W + r * ldw + c * 8;
    uint8_t *mo = mask ? mask + r * ldm + c * 8 : nullptr;
    unsigned n = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool k = (bits >> j) & 1u;
        uint16_t wj = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) wj = (k && n == unsigned(s)) ? v[s] : wj;   // a fifth set bit of a bad byte selects nothing
        o[j] = wj;
        if (mo) mo[j] = uint8_t(k);
        n += k;
    }
}

}  // namespace vlmc

using namespace vlmc;

extern "C" int vlmc_pack_48(const void *W, int dtype, int64_t out_features, int64_t in_features, int64_t ldw, const uint8_t *mask, int64_t ldm,
                            void *values, uint8_t *meta, unsigned int *bad_groups, void *stream) {
    VLMC_REQUIRE(dtype == VLMC_F16 || dtype == VLMC_BF16, "vlmc_pack_48: dtype must be VLMC_F16 or VLMC_BF16");
    VLMC_REQUIRE(W && mask && values && meta && bad_groups, "vlmc_pack_48: null pointer");
    VLMC_REQUIRE(out_features > 0 && in_features > 0 && in_features % 8 == 0, "vlmc_pack_48: in_features must be a positive multiple of 8");
    VLMC_REQUIRE(ldw >= in_features && ldm >= in_features && out_features * (in_features / 8) < (int64_t(1) << 39), "vlmc_pack_48: bad shape");
    const int64_t n = out_features * (in_features / 8);
    hipLaunchKernelGGL(pack48_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, as_stream(stream), static_cast<const uint16_t *>(W), ldw, mask,
                       ldm, out_features, in_features, static_cast<uint16_t *>(values), meta, bad_groups);
    VLMC_HIP_CHECK_LAUNCH("vlmc_pack_48");
    return VLMC_OK;
}

extern "C" int vlmc_unpack_48(const void *values, const uint8_t *meta, int dtype, int64_t out_features, int64_t in_features, void *W, int64_t ldw,
                              uint8_t *mask, int64_t ldm, unsigned int *bad_groups, void *stream) {
    VLMC_REQUIRE(dtype == VLMC_F16 || dtype == VLMC_BF16, "vlmc_unpack_48: dtype must be VLMC_F16 or VLMC_BF16");
    VLMC_REQUIRE(W && values && meta && bad_groups, "vlmc_unpack_48: null pointer");
    VLMC_REQUIRE(out_features > 0 && in_features > 0 && in_features % 8 == 0, "vlmc_unpack_48: in_features must be a positive multiple of 8");
    VLMC_REQUIRE(ldw >= in_features && (!mask || ldm >= in_features) && out_features * (in_features / 8) < (int64_t(1) << 39), "vlmc_unpack_48: bad shape");
    const int64_t n = out_features * (in_features / 8);
    hipLaunchKernelGGL(unpack48_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, as_stream(stream), static_cast<const uint16_t *>(values), meta,
                       out_features, in_features, static_cast<uint16_t *>(W), ldw, mask, ldm, bad_groups);
    VLMC_HIP_CHECK_LAUNCH("vlmc_unpack_48");
    return VLMC_OK;
}
