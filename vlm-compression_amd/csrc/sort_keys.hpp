// Order-preserving unsigned keys of fp32 values: the keys compare as integers the way torch.sort orders the floats (NaN last).
// score_select.hip (the multi-tensor global threshold) produces the same order as signed_key() by another design, kept in its
// file: the key of every element is never formed; prefixes and thresholds are compared on the scores' canonical raw bits.
#pragma once
#include "common.hpp"

namespace vlmc {

// A score that is >= +0 or NaN (Wanda's |w| * sqrt(s), SparseGPT's w^2 / d^2).
// NaN sorts last (torch.sort semantics) -> 0xFFFFFFFF; -0 (impossible, but harmless) == +0.
__device__ __forceinline__ uint32_t score_key(float sc) {
    return (sc != sc) ? 0xFFFFFFFFu : (__float_as_uint(sc) & 0x7FFFFFFFu);
}

// The same score inside the streaming passes of wanda_select.hip: clearing the sign bit orders every finite score
// and +inf like score_key() and leaves NaNs above +inf (0x7F800001..0x7FFFFFFF) -- one instruction.  A bin that
// reaches above +inf is handed to the fallback, which uses score_key()'s single NaN key.
__device__ __forceinline__ uint32_t stream_key(float sc) { return __float_as_uint(sc) & 0x7FFFFFFFu; }

// A signed float for ascending sorts (DSnoT's regrowing metric): -0 == +0, NaN last.
__device__ __forceinline__ uint32_t signed_key(float x) {
    if (x != x) return 0xFFFFFFFFu;
    x = x + 0.f;                                             // -0 -> +0
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

}  // namespace vlmc
