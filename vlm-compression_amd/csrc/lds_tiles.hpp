// LDS tile helpers shared by the kernels that keep 16-bit operand tiles in rows of 64 elements = 128 B (gemm_nt.hip,
// lora_gemm.hip, attn_matmul.hip) and by everything that stages through the LDS-DMA (those, sdpa_kernel.hpp,
// attn_fused_kernel.hpp): the swizzled byte offsets and the one load the compiler does not see.
#pragma once
#include "common.hpp"

namespace vlmc {

constexpr int LDS_ROW_BYTES = 128;

// [rows][64 k] image: byte offset of 16-B chunk `ch` (0..7) of tile row `row`, the chunk index XOR-ed with row & 7 -- the
// 16-row x 4-chunk fragment reads (ds_read_b128) are bank-conflict free
__device__ __forceinline__ int row_off(int row, int ch) { return row * LDS_ROW_BYTES + ((ch ^ (row & 7)) << 4); }
// [64 k][64 n] image of an NN operand for the transposing reads: a 32-lane half reads rows q, 8 + q (q = 0..3) of one
// 16-column block -- chunk pairs XOR-ed with (k & 3) | ((k >> 3) & 1) << 2 put its eight 32-byte pieces on all 64 banks once
__device__ __forceinline__ int tr_swz(int k) { return (k & 3) | (((k >> 3) & 1) << 2); }
__device__ __forceinline__ int tr_off(int k, int ch) { return k * LDS_ROW_BYTES + ((ch ^ tr_swz(k)) << 4); }

// 64 lanes x 16 B from global memory straight into 1 KiB of LDS at `lds_addr` (wave-uniform), lane l at lds_addr + 16 l.
// hipcc knows nothing of this load: whoever issues it counts its own vmcnt.
__device__ __forceinline__ void glds16(const void *gptr, uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_addr), "v"(gptr) : "memory", "m0");
}

}  // namespace vlmc
