// instantiations of csrc/attn_fused_kernel.hpp: bf16, 2 addend(s), with the clamp of modeling_llama.py:236 (vlmc_attn_fwd_clamp)
#include "attn_fused_kernel.hpp"

namespace vlmc {
int attn_dispatch_clamp_bf16_2(const AttnArgs &a, int64_t bh, int ds, hipStream_t s) { return attn_dispatch<bf16_t, 2, true>(a, bh, ds, s); }
}  // namespace vlmc
