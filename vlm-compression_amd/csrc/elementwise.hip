// vlmc_gelu: the activation of a replayed block's feed-forward with ONE instruction sequence for every element.
//
// `self.act(self.fc1(x))` (eva_vit.py:62-64, nn.GELU()), the gated GELU of T5 v1.1 (modeling_t5.py:337-346) run through torch's
// elementwise kernels, and those compute a tensor's LAST partial block of 2048 elements with other code than its body: in the tail
// hipcc contracts x/2 * (1 + erf(x / sqrt 2)) into fma(x/2, erf, x/2) -- gelu(-6.7) is +0.0 there and -0.0 in the body, ~20 % of all
// fp16 inputs differ in the last bit (tools/micro/gelu_variants.py).  Which rows of a batch are "the tail" depends on how many
// samples share the forward: a sample's last rows get other bits alone than in a group -- the one elementwise op of the blocks that
// is not batch-invariant in torch.  Here every element takes the BODY's arithmetic (all 65 536 fp16 / bf16 inputs equal torch's body
// bit for bit: tests/test_gelu_gpu.py), whatever its position.  HBM-bound: 16 B per lane and step, 2 + 2 bytes per element.
#include <type_traits>

#include "common.hpp"
#include "mfma.hpp"

namespace vlmc {

// at::native::GeluCUDAKernelImpl: opmath float;  none: x * 0.5 * (1 + erf(x * M_SQRT1_2));
// tanh: 0.5 * x * (1 + tanh(kBeta * (x + kKappa * x^3))), kBeta = M_SQRT2 * M_2_SQRTPI * 0.5, kKappa = 0.044715
template <typename T, int TANH> __device__ __forceinline__ uint16_t gelu_one(uint16_t v) {
    const float x = to_f32<T>(v);
    float y;
    if (TANH) {
        constexpr float kBeta = 1.41421356237309504880f * 1.12837916709551257390f * 0.5f, kKappa = 0.044715f;
        const float x3 = ieee_mul(ieee_mul(x, x), x);
        const float inner = ieee_mul(kBeta, ieee_add(x, ieee_mul(kKappa, x3)));
        y = ieee_mul(ieee_mul(0.5f, x), ieee_add(1.0f, tanhf(inner)));
    } else {
        y = ieee_mul(ieee_mul(x, 0.5f), ieee_add(1.0f, erff(ieee_mul(x, 0.70710678118654752440f))));
    }
    asm volatile("" : "+v"(y));                                            // (an fp32 value of its own, rounded to the dtype afterwards)
    return from_f32<T>(y);
}

template <typename T, int TANH>
__global__ __launch_bounds__(256) void gelu_kernel(const uint16_t *__restrict__ x, uint16_t *__restrict__ y, int64_t n, int vec) {
    const int64_t chunks = (n + 7) / 8;
    for (int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x; c < chunks; c += int64_t(gridDim.x) * 256) {
        const int64_t e0 = c * 8;
        uint16_t e[8];
        if (vec && e0 + 8 <= n) {
            const u32x4_t v = *reinterpret_cast<const u32x4_t *>(x + e0);
            __builtin_memcpy(e, &v, 16);
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = gelu_one<T, TANH>(e[j]);
            u32x4_t o;
            __builtin_memcpy(&o, e, 16);
            *reinterpret_cast<u32x4_t *>(y + e0) = o;
        } else {
            for (int j = 0; j < 8 && e0 + j < n; ++j) y[e0 + j] = gelu_one<T, TANH>(x[e0 + j]);
        }
    }
}

// vlmc_gelu_mul: T5 v1.1's gated product `F.gelu(wi_0(h)) * wi_1(h)` (modeling_t5.py:337-341) in one pass.  The GELU is gelu_one,
// rounded to the dtype as `vlmc_gelu` stores it; the product is torch's 16-bit `mul` (opmath float, one rounding; torch's fp32 ->
// bf16 conversion answers every NaN with 0x7FC0, the hardware conversion keeps sign and payload).
template <typename T, int TANH> __device__ __forceinline__ uint16_t gelu_mul_one(uint16_t xv, uint16_t yv) {
    float p = ieee_mul(to_f32<T>(gelu_one<T, TANH>(xv)), to_f32<T>(yv));
    asm volatile("" : "+v"(p));
    if (std::is_same<T, bf16_t>::value && p != p) return uint16_t(0x7FC0);
    return from_f32<T>(p);
}

// Rows of x / y / out are `cols` elements at pitches ldx / ldy / ldo; a lane takes 8 consecutive columns of one row per step.  Step
// i of the launch works on row rowmap[i] (i itself without a map): the first n_real of them are computed, the others get zeros in
// `out` and are not read.  `vec`: every pointer 16-byte aligned and every pitch a multiple of 8, so that a whole step is one 16-byte
// access per operand; a row's last partial step and everything of an unaligned call go element by element -- the same arithmetic.
template <typename T, int TANH>
__global__ __launch_bounds__(256) void gelu_mul_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ y, uint16_t *__restrict__ out,
                                                       int64_t rows, int64_t cols, int64_t ldx, int64_t ldy, int64_t ldo,
                                                       const int32_t *__restrict__ rowmap, int64_t n_real, int vec) {
    const int64_t per_row = (cols + 7) / 8, chunks = rows * per_row;
    for (int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x; c < chunks; c += int64_t(gridDim.x) * 256) {
        // (a launch of fewer than 2^32 steps -- every one of the replay's -- divides in 32 bits)
        const int64_t i = chunks <= 0xffffffffll ? int64_t(uint32_t(c) / uint32_t(per_row)) : c / per_row;
        const int64_t e0 = (c - i * per_row) * 8;
        const int64_t r = rowmap ? int64_t(rowmap[i]) : i;
        const bool whole = vec && e0 + 8 <= cols;
        uint16_t *o = out + r * ldo + e0;
        if (i >= n_real) {                                                 // a padding row: zeros, nothing read
            if (whole) *reinterpret_cast<u32x4_t *>(o) = u32x4_t{0u, 0u, 0u, 0u};
            else for (int j = 0; j < 8 && e0 + j < cols; ++j) o[j] = 0;
            continue;
        }
        const uint16_t *xr = x + r * ldx + e0, *yr = y + r * ldy + e0;
        if (whole) {
            const u32x4_t xv = *reinterpret_cast<const u32x4_t *>(xr), yv = *reinterpret_cast<const u32x4_t *>(yr);
            uint16_t a[8], b[8];
            __builtin_memcpy(a, &xv, 16);
            __builtin_memcpy(b, &yv, 16);
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = gelu_mul_one<T, TANH>(a[j], b[j]);
            u32x4_t ov;
            __builtin_memcpy(&ov, a, 16);
            *reinterpret_cast<u32x4_t *>(o) = ov;
        } else {
            for (int j = 0; j < 8 && e0 + j < cols; ++j) o[j] = gelu_mul_one<T, TANH>(xr[j], yr[j]);
        }
    }
}

// fp32 tensors (the reference's Q-Former stays in fp32, blip2_t5_instruct.py:76-95): the same body arithmetic, nothing to round
template <int TANH>
__global__ __launch_bounds__(256) void gelu_f32_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t n, int vec) {
    const int64_t chunks = (n + 3) / 4;
    for (int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x; c < chunks; c += int64_t(gridDim.x) * 256) {
        const int64_t e0 = c * 4;
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        const bool whole = vec && e0 + 4 <= n;
        if (whole) {
            const u32x4_t v = *reinterpret_cast<const u32x4_t *>(x + e0);
            __builtin_memcpy(e, &v, 16);
        } else {
            for (int j = 0; j < 4 && e0 + j < n; ++j) e[j] = x[e0 + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = e[j];
            float r;
            if (TANH) {
                constexpr float kBeta = 1.41421356237309504880f * 1.12837916709551257390f * 0.5f, kKappa = 0.044715f;
                const float x3 = ieee_mul(ieee_mul(v, v), v);
                r = ieee_mul(ieee_mul(0.5f, v), ieee_add(1.0f, tanhf(ieee_mul(kBeta, ieee_add(v, ieee_mul(kKappa, x3))))));
            } else {
                r = ieee_mul(ieee_mul(v, 0.5f), ieee_add(1.0f, erff(ieee_mul(v, 0.70710678118654752440f))));
            }
            e[j] = r;
        }
        if (whole) {
            u32x4_t o;
            __builtin_memcpy(&o, e, 16);
            *reinterpret_cast<u32x4_t *>(y + e0) = o;
        } else {
            for (int j = 0; j < 4 && e0 + j < n; ++j) y[e0 + j] = e[j];
        }
    }
}

}  // namespace vlmc

using namespace vlmc;

extern "C" int vlmc_gelu(const void *x, void *y, int64_t n, int dtype, int tanh_approx, void *stream) {
    VLMC_REQUIRE(dtype == VLMC_F16 || dtype == VLMC_BF16 || dtype == VLMC_F32, "vlmc_gelu: dtype must be VLMC_F16, VLMC_BF16 or VLMC_F32");
    VLMC_REQUIRE(x && y && n >= 0, "vlmc_gelu: null pointer or negative size");
    VLMC_REQUIRE(tanh_approx == 0 || tanh_approx == 1, "vlmc_gelu: tanh_approx must be 0 (erf) or 1 (tanh)");
    if (n == 0) return VLMC_OK;
    const int vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0;
    int64_t blocks = ((n + 7) / 8 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const dim3 grid{unsigned(blocks)}, block{256};
    hipStream_t s = as_stream(stream);
    if (dtype == VLMC_F32) {
        if (tanh_approx) hipLaunchKernelGGL((gelu_f32_kernel<1>), grid, block, 0, s, static_cast<const float *>(x), static_cast<float *>(y), n, vec);
        else hipLaunchKernelGGL((gelu_f32_kernel<0>), grid, block, 0, s, static_cast<const float *>(x), static_cast<float *>(y), n, vec);
        VLMC_HIP_CHECK_LAUNCH("vlmc_gelu");
        return VLMC_OK;
    }
    const uint16_t *xi = static_cast<const uint16_t *>(x);
    uint16_t *yo = static_cast<uint16_t *>(y);
    if (dtype == VLMC_F16) {
        if (tanh_approx) hipLaunchKernelGGL((gelu_kernel<f16_t, 1>), grid, block, 0, s, xi, yo, n, vec);
        else hipLaunchKernelGGL((gelu_kernel<f16_t, 0>), grid, block, 0, s, xi, yo, n, vec);
    } else {
        if (tanh_approx) hipLaunchKernelGGL((gelu_kernel<bf16_t, 1>), grid, block, 0, s, xi, yo, n, vec);
        else hipLaunchKernelGGL((gelu_kernel<bf16_t, 0>), grid, block, 0, s, xi, yo, n, vec);
    }
    VLMC_HIP_CHECK_LAUNCH("vlmc_gelu");
    return VLMC_OK;
}

extern "C" int vlmc_gelu_mul(const void *x, const void *y, void *out, int dtype, int tanh_approx, int64_t rows, int64_t cols, int64_t ldx,
                             int64_t ldy, int64_t ldo, const int32_t *rowmap, int64_t n_real, void *stream) {
    VLMC_REQUIRE(dtype == VLMC_F16 || dtype == VLMC_BF16, "vlmc_gelu_mul: dtype must be VLMC_F16 or VLMC_BF16");
    VLMC_REQUIRE(x && y && out, "vlmc_gelu_mul: null pointer");
    VLMC_REQUIRE(tanh_approx == 0 || tanh_approx == 1, "vlmc_gelu_mul: tanh_approx must be 0 (erf) or 1 (tanh)");
    VLMC_REQUIRE(rows >= 0 && cols >= 0 && rows <= INT32_MAX && cols <= INT32_MAX, "vlmc_gelu_mul: rows and cols must be in 0 .. 2^31 - 1");
    VLMC_REQUIRE(ldx >= cols && ldy >= cols && ldo >= cols, "vlmc_gelu_mul: a row pitch is smaller than cols");
    VLMC_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out)) & 1u) == 0,
                 "vlmc_gelu_mul: x, y and out must be 2-byte aligned");
    if (rowmap) VLMC_REQUIRE(n_real >= 0 && n_real <= rows && (reinterpret_cast<uintptr_t>(rowmap) & 3u) == 0,
                             "vlmc_gelu_mul: 0 <= n_real <= rows and a 4-byte aligned rowmap expected");
    else n_real = rows;
    if (rows == 0 || cols == 0) return VLMC_OK;
    const int vec = aligned16(x) && aligned16(y) && aligned16(out) && ldx % 8 == 0 && ldy % 8 == 0 && ldo % 8 == 0;
    int64_t blocks = (rows * ((cols + 7) / 8) + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const dim3 grid{unsigned(blocks)}, block{256};
    hipStream_t s = as_stream(stream);
    const uint16_t *xi = static_cast<const uint16_t *>(x), *yi = static_cast<const uint16_t *>(y);
    uint16_t *oo = static_cast<uint16_t *>(out);
    if (dtype == VLMC_F16) {
        if (tanh_approx) hipLaunchKernelGGL((gelu_mul_kernel<f16_t, 1>), grid, block, 0, s, xi, yi, oo, rows, cols, ldx, ldy, ldo, rowmap, n_real, vec);
        else hipLaunchKernelGGL((gelu_mul_kernel<f16_t, 0>), grid, block, 0, s, xi, yi, oo, rows, cols, ldx, ldy, ldo, rowmap, n_real, vec);
    } else {
        if (tanh_approx) hipLaunchKernelGGL((gelu_mul_kernel<bf16_t, 1>), grid, block, 0, s, xi, yi, oo, rows, cols, ldx, ldy, ldo, rowmap, n_real, vec);
        else hipLaunchKernelGGL((gelu_mul_kernel<bf16_t, 0>), grid, block, 0, s, xi, yi, oo, rows, cols, ldx, ldy, ldo, rowmap, n_real, vec);
    }
    VLMC_HIP_CHECK_LAUNCH("vlmc_gelu_mul");
    return VLMC_OK;
}
