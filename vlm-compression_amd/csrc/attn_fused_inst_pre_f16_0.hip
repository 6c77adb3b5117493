// instantiations of csrc/attn_fused_kernel.hpp: f16, 0 addend(s), with the operand pre-ops of eva_vit.py:133-141 (vlmc_attn_fwd_pre)
#include "attn_fused_kernel.hpp"

namespace vlmc {
int attn_dispatch_pre_f16_0(const AttnArgs &a, int64_t bh, int ds, hipStream_t s) { return attn_dispatch<f16_t, 0, false, true>(a, bh, ds, s); }
}  // namespace vlmc
