// Wave-wide primitives of the selection kernels (wanda_select.hip, dsnot.hip, dsnot_lists.hpp, sparsegpt.hip) and the row
// reductions (row_reduce.hip), one definition each.  Where two mechanisms remain the name says which: _dpp (no LDS traffic, a row
// of 16 lanes per step) or _shfl (ds_bpermute).  The integer pairs compute the same value and stay apart only because swapping
// them moves registers in kernels at an occupancy step.  The float sums differ in the ORDER of their additions: that is behaviour.
#pragma once
#include "common.hpp"

namespace vlmc {

// ---- integer sums (result wave-uniform / valid in every lane) ---------------------------------------------------------------
// (after the four DPP steps every lane holds the total of its row of 16 lanes; the four row totals meet through readlane)
__device__ __forceinline__ uint32_t wave_sum_u32_dpp(uint32_t v) {
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x141, 0xF, 0xF, true));  // row_half_mirror
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x140, 0xF, 0xF, true));  // row_mirror
    return uint32_t(__builtin_amdgcn_readlane(int(v), 0)) + uint32_t(__builtin_amdgcn_readlane(int(v), 16)) +
           uint32_t(__builtin_amdgcn_readlane(int(v), 32)) + uint32_t(__builtin_amdgcn_readlane(int(v), 48));
}
__device__ __forceinline__ uint32_t wave_sum_u32_shfl(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// ---- float sums: deterministic, but they differ in the last bit on some inputs -- a caller keeps the order it has ---------------
// fp64 butterfly (lanes l and l ^ 32, then ^ 16 .. ^ 1): the score partial sums of wanda_select.hip's streaming passes.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}
// fp32 butterfly, same lane order, every addition one IEEE add.  This IS vlmc_row_mean's definition of a row's mean (lane partials
// in ascending i, this tree, one division): row_mean_kernel and rms_norm_kernel (row_reduce.hip) share it bit for bit.
__device__ __forceinline__ float wave_sum_f32_shfl(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = ieee_add(v, __shfl_xor(v, off, kWave));
    return v;
}
// fp32 by DPP, the four row totals combined PAIRWISE: (r0 + r1) + (r2 + r3).  select_row_body (wanda_select.hip: the SEL_ROW
// kernels and the mixed-width launch) sums a row's scores with it before the waves' totals are added in fp64.
__device__ __forceinline__ float wave_sum_f32_dpp_pairwise(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true));
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (r0 + r1) + (r2 + r3);
}
// fp32 by DPP, the four row totals combined IN ORDER: ((r0 + r1) + r2) + r3.  DSnoT's reconstruction error of a row -- the sum
// of D = w * mean over the pruned columns, whose SIGN decides which list every cycle reads (dsnot_pruner.py:407-751) -- is
// summed with it by dsnot_simulate_kernel (dsnot.hip) and by the list kernel (dsnot_lists.hpp).  The two are each other's
// cross-check, event for event (tests/test_dsnot_gpu.py), so both keep this order; a row whose error is within an ulp of zero
// changes its mask if the order does.
__device__ __forceinline__ float wave_sum_f32_dpp_inorder(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)) +
           __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16)) +
           __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)) +
           __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
}

// ---- inclusive prefix sum over the lanes: DPP row shifts + row broadcasts, or shuffles -----------------------------------------
__device__ __forceinline__ uint32_t wave_incl_scan_u32_dpp(uint32_t v) {
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xF, 0xF, false));   // row_shr:1
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xF, 0xF, false));   // row_shr:2
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xF, 0xF, false));   // row_shr:4
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xF, 0xF, false));   // row_shr:8
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xA, 0xF, false));   // row_bcast:15 -> rows 1,3
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xC, 0xF, false));   // row_bcast:31 -> rows 2,3
    return v;
}
// (sparsegpt.hip's select-sweep: one scan per radix level)
__device__ __forceinline__ uint32_t wave_incl_scan_u32_shfl(uint32_t v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = uint32_t(__shfl_up(int(v), off, 64));
        if (int(threadIdx.x & 63) >= off) v += o;
    }
    return v;
}

// ---- rank search over a histogram held PER consecutive bins per thread ----------------------------------------------------------
// The last step of every such search (block_find_rank / block_find_rank2 in wanda_select.hip, sel_find_rank in sparsegpt.hip),
// by the one thread whose bins hold the rank: `cum` comes in as the count before the thread's first bin and leaves as the count
// before the bin returned, the one with cum <= need < cum + h[bin].  Wave 0 of dl_radix_kth (dsnot_lists.hpp) keeps the same
// loop written out: calling this instead changed the generated code of the list kernels (profiles/wave_ops_refactor.md).
template <int PER> __device__ __forceinline__ int walk_bins(const uint32_t (&h)[PER], uint32_t need, uint32_t &cum) {
    int i = 0;
    for (; i < PER - 1; ++i) {
        if (cum + h[i] > need) break;
        cum += h[i];
    }
    return i;
}

// ---- min / max of a 32-bit unsigned (result valid in every lane) -----------------------------------------------------------
__device__ __forceinline__ uint32_t wave_max_u32_dpp(uint32_t v) {
    v = max(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0xB1, 0xF, 0xF, true)));
    v = max(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x4E, 0xF, 0xF, true)));
    v = max(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x141, 0xF, 0xF, true)));
    v = max(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x140, 0xF, 0xF, true)));
    return max(max(uint32_t(__builtin_amdgcn_readlane(int(v), 0)), uint32_t(__builtin_amdgcn_readlane(int(v), 16))),
               max(uint32_t(__builtin_amdgcn_readlane(int(v), 32)), uint32_t(__builtin_amdgcn_readlane(int(v), 48))));
}
__device__ __forceinline__ uint32_t wave_min_u32_dpp(uint32_t v) { return ~wave_max_u32_dpp(~v); }
__device__ __forceinline__ uint32_t wave_min_u32_shfl(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = uint32_t(__shfl_xor(int(v), off, 64));
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32_shfl(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = uint32_t(__shfl_xor(int(v), off, 64));
        v = o > v ? o : v;
    }
    return v;
}

// ---- register pins -----------------------------------------------------------------------------------------------------------
// The compiler otherwise keeps every per-element predicate (a 64-bit lane mask each) and every bin index of one pass alive
// for the next pass over the same registers: hundreds of spilled SGPRs and 2x the VGPRs (occupancy 1-2 waves per SIMD).  A
// pass starts from an opaque copy of its mask / range so that what it needs is recomputed (two instructions per element).
__device__ __forceinline__ uint32_t opaque(uint32_t v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ uint32_t uniform(uint32_t v) {             // a wave-uniform value, held in an SGPR
    v = uint32_t(__builtin_amdgcn_readfirstlane(int(v)));
    asm volatile("" : "+s"(v));
    return v;
}

// ---- workgroup syncs that order LDS traffic: two forms, named after their callers, NOT interchangeable ------------------------
//                  NW > 1                                                         NW == 1 (one wave: program order suffices)
//   row_sync<NW>   lds_barrier(): release / s_barrier / acquire on LDS only       release fence + wave_barrier, no acquire fence
//   dl_sync<NW>    __syncthreads(): waits for vmcnt as well                       release fence + wave_barrier + acquire fence
// row_sync (select_row_body, wanda_select.hip): the row kernels have global loads and non-temporal stores in flight across their
// syncs; __syncthreads() would drain them (s_waitcnt vmcnt(0)) at every radix sweep.  One wave's LDS operations complete in issue
// order, so its one-wave form only has to keep the compiler from moving the reads above the atomics: nothing is made to wait.
// dl_sync (dsnot_lists.hpp) is the plain full barrier, and its one-wave form carries both fences, so both forms order everything
// before the sync against everything after it.  The list kernels' registers were tuned with these waits in place (see the
// occupancy notes in dsnot_lists.hpp): one more reason not to give them row_sync's lighter form unmeasured.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
template <int NW> __device__ __forceinline__ void row_sync() {
    if constexpr (NW > 1) {
        lds_barrier();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}
template <int NW> __device__ __forceinline__ void dl_sync() {
    if constexpr (NW > 1) __syncthreads();
    else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

}  // namespace vlmc
