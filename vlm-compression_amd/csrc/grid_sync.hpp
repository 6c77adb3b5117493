// The grid barrier of the kernels whose workgroups must agree inside one launch: matrix_fused_kernel (wanda_select.hip) and
// the select-sweep of sparsegpt.hip.  One arrival counter per barrier, device-scope atomics only (no L2 write-back fences).
//
// The grid never exceeds one workgroup per CU, so every workgroup is resident on an otherwise idle GPU.  If they are not (CUs
// held by another stream), the bounded spin runs out and a waiter raises the counter's fail bit.  The fail bit can only be set
// (compare-and-swap) while the count is still short, and whoever arrives or polls afterwards sees it before the count: EITHER
// EVERY WORKGROUP PASSES THE BARRIER OR NONE DOES.  Past a failed barrier nobody writes a result; the caller's last workgroup
// to finish (its own done counter) does the whole job alone by the streaming route.  Every wave therefore reaches the end of
// the kernel whatever the residency.  The counter must be zero on entry; the caller's last workgroup zeroes it again.
// The library's third spin loop, wait_flag / publish in chol_persistent.hip, follows a different protocol (a flag per tile
// plus an abort word) and stays there.
#pragma once
#include "common.hpp"

namespace vlmc {

constexpr uint32_t kGridBarFail = 0x80000000u;   // fail bit of an arrival counter
constexpr uint32_t kGridSpinMax = 1u << 12;      // x (device-scope load + s_sleep, ~2.2 us) ~ 9 ms; a barrier normally takes < 20 us

__device__ __forceinline__ uint32_t ld_dev(const uint32_t *p) {       // device-scope load (bypasses the CU's L1)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// tid 0 of a workgroup: arrive at the counter and wait for `n` arrivals.  false = the barrier failed (for every workgroup).
__device__ __forceinline__ bool grid_arrive_wait(uint32_t *ctr, uint32_t n) {
    uint32_t v = atomicAdd(ctr, 1u) + 1u;
    for (uint32_t it = 0;; ++it) {
        if (v & kGridBarFail) return false;
        if (v >= n) return true;
        if (it >= kGridSpinMax) {                                // give up: declare the failure unless it completed meanwhile
            const uint32_t seen = atomicCAS(ctr, v, v | kGridBarFail);
            if (seen == v) return false;
            v = seen;
            continue;
        }
        __builtin_amdgcn_s_sleep(8);
        v = ld_dev(ctr);
    }
}

}  // namespace vlmc
