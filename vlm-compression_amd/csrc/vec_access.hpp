// 16-byte access to rows of 16-bit elements that are only 2-byte aligned (a head's slice of a fused QKV tensor, a row of odd
// pitch), the all-zero chunk that padding is "loaded" from, and the one rounding of an fp32 value to the 16-bit dtype.
// Shared by attn_matmul.hip, sdpa_kernel.hpp, attn_fused_kernel.hpp, rope.hip and lora_gemm.hip.
#pragma once
#include "common.hpp"
#include "mfma.hpp"

namespace vlmc {

// the packed struct makes the compiler emit a load / store that is legal at any 2-byte boundary
struct __attribute__((packed, aligned(2))) U16x8 { u32x4_t v; };
struct __attribute__((packed, aligned(2))) U16x4 { uint32_t lo, hi; };     // 8 bytes likewise
__device__ __forceinline__ u32x4_t load16_a2(const uint16_t *p) { return reinterpret_cast<const U16x8 *>(p)->v; }
__device__ __forceinline__ void store16_a2(uint16_t *p, u32x4_t v) { reinterpret_cast<U16x8 *>(p)->v = v; }

__device__ __attribute__((aligned(16))) const uint32_t zero_chunk[4] = {0u, 0u, 0u, 0u};      // what padding is "loaded" from

// the bits of one rounding to the dtype, as an fp32 value again
template <typename T> __device__ __forceinline__ float round16(float v) { return to_f32<T>(from_f32<T>(v)); }

}  // namespace vlmc
