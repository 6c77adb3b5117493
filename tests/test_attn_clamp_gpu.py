"""GPU: `vlmc_attn_fwd_clamp` -- the attention chain of the reference's LLaMA layer (modeling_llama.py:222-240: `matmul / sqrt(d)`,
`+ attention_mask`, `torch.max(.., torch.tensor(finfo.min))`, fp32 softmax, `matmul`) in one launch -- against the SAME chain op by op
on this library's unfused kernels (`vlmc_attn_matmul`, torch's `/`, `+`, `torch.max`, `vlmc_softmax_rows`): bit for bit, as
tests/test_attn_fused_gpu.py does for the chains without a clamp.  Vicuna shapes (32 heads of 128), fp16 and bf16, masks that hold
-inf, with and without per-sample lengths; and against fp64 attention, where the fused kernel's error may not exceed the unfused
sequence's (they are the same bits: an equality in disguise that also guards this file's own reference)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, D = 32, 128


def _bits(t):
    return t.contiguous().view(torch.int16)


def _heads(B, T, dtype, g, scale=1.0, heads=H, d=D):
    return (torch.randn(B, T, heads * d, generator=g, device=DEV) * scale).to(dtype).view(B, T, heads, d).transpose(1, 2)


def _llama_mask(lens, T, dtype):
    """`_prepare_decoder_attention_mask` (modeling_llama.py:470-491) of a right-padded batch: the causal mask PLUS the expanded padding
    mask, both at the dtype's minimum -- -inf where a key is padded AND causally hidden"""
    from vlmc.synthetic_llama import prepare_decoder_attention_mask
    atts = torch.zeros(len(lens), T, dtype=torch.bool, device=DEV)
    for i, n in enumerate(lens):
        atts[i, :n] = True
    return prepare_decoder_attention_mask(atts, (len(lens), T), dtype, DEV)


def _unfused(q, k, v, mask, lo):
    from vlmc import ops
    s = ops.attn_matmul(q, k.transpose(2, 3)) / math.sqrt(q.shape[-1])
    s = s + mask
    s = torch.max(s, torch.tensor(lo))                                      # a 0-dim CPU tensor, as the reference writes it
    p = ops.softmax_rows(s, torch.float32).to(q.dtype)                      # softmax(dim=-1, dtype=torch.float32).to(dtype)
    return ops.attn_matmul(p, v)


def _mul(d):
    import numpy as np
    return float(np.float32(1.0) / np.float32(math.sqrt(d)))               # torch divides by a number as a product with the fp32 reciprocal


def _fp64(q, k, v, mask, lo):
    s = q.double() @ k.double().transpose(2, 3) / math.sqrt(q.shape[-1]) + mask.double()
    return torch.softmax(torch.clamp(s, min=float(lo)), -1) @ v.double()


CASES = [(dtype, T, lens) for dtype in (torch.float16, torch.bfloat16)
         for T, lens in ((40, [40, 17, 33]), (100, [100, 61]), (176, [176, 40, 129]), (288, [288, 200]))]


@pytest.mark.parametrize("dtype,T,lens", CASES, ids=[f"{'fp16' if c[0] == torch.float16 else 'bf16'}-T{c[1]}" for c in CASES])
def test_clamped_chain_has_the_bits_of_the_unfused_sequence(dtype, T, lens):
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(T)
    B = len(lens)
    q, k, v = _heads(B, T, dtype, g, 0.6), _heads(B, T, dtype, g, 0.6), _heads(B, T, dtype, g)
    mask = _llama_mask(lens, T, dtype)
    lo = torch.finfo(dtype).min
    assert bool(torch.isinf(mask).any()), "the mask of a right-padded batch must hold -inf (min + min) in 16 bits"
    want = _unfused(q, k, v, mask, lo)
    got = ops.attn_fused_clamp(q, k, v, _mul(D), [mask], lo)
    assert got.shape == want.shape == (B, H, T, D) and got.transpose(1, 2).is_contiguous()
    nd = int((_bits(got) != _bits(want)).sum())
    ref = _fp64(q, k, v, mask, lo)
    err_fused, err_unfused = float((got.double() - ref).abs().max()), float((want.double() - ref).abs().max())
    print(f"clamp {dtype} T={T}: {nd} of {got.numel()} entries differ; max error against fp64: fused {err_fused:.3e}, unfused {err_unfused:.3e}")
    assert nd == 0
    assert bool(torch.isfinite(got.float()).all())                          # (without the clamp a fully masked row would be NaN)
    assert err_fused <= err_unfused
    # per-sample lengths: live rows keep the bits of the full launch, the others are zero
    ql = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for kw in (dict(q_len=ql, k_len=ql), dict(k_len=ql), dict(q_len=ql)):
        cut = ops.attn_fused_clamp(q, k, v, _mul(D), [mask], lo, **kw)
        for i, n in enumerate(lens):
            assert torch.equal(_bits(cut[i, :, :n]), _bits(got[i, :, :n])), (list(kw), i)
            if "q_len" in kw:
                assert bool((_bits(cut[i, :, n:]) == 0).all()), "a padding query is not +0"


def test_clamp_of_a_padded_group_equals_each_sample_alone():
    """what the replay engine relies on: a sample inside a padded group (its mask padded with the dtype's minimum, lengths handed to the
    kernel) has the bits of the sample forwarded alone with its own [1, 1, T, T] mask"""
    from vlmc import ops
    from vlmc.synthetic_llama import prepare_decoder_attention_mask
    dtype, lens = torch.float16, [48, 176, 77, 60]
    T, lo = max(lens), torch.finfo(torch.float16).min
    g = torch.Generator(device=DEV).manual_seed(7)
    q, k, v = _heads(len(lens), T, dtype, g, 0.6), _heads(len(lens), T, dtype, g, 0.6), _heads(len(lens), T, dtype, g)
    mask = torch.full((len(lens), 1, T, T), lo, dtype=dtype, device=DEV)
    own = []
    for i, n in enumerate(lens):
        m = prepare_decoder_attention_mask(torch.ones(1, n, dtype=torch.bool, device=DEV), (1, n), dtype, DEV)
        mask[i, :, :n, :n] = m[0]
        own.append(m)
    ql = torch.tensor(lens, dtype=torch.int32, device=DEV)
    group = ops.attn_fused_clamp(q, k, v, _mul(D), [mask], lo, q_len=ql, k_len=ql)
    for i, n in enumerate(lens):
        alone = ops.attn_fused_clamp(q[i:i + 1, :, :n], k[i:i + 1, :, :n], v[i:i + 1, :, :n], _mul(D), [own[i]], lo)
        assert torch.equal(_bits(group[i:i + 1, :, :n]), _bits(alone)), i


def test_nan_scores_stay_nan_and_two_addends():
    from vlmc import ops
    dtype, T, lo = torch.bfloat16, 40, torch.finfo(torch.bfloat16).min
    g = torch.Generator(device=DEV).manual_seed(11)
    q, k, v = _heads(2, T, dtype, g, 0.6, 4, 64), _heads(2, T, dtype, g, 0.6, 4, 64), _heads(2, T, dtype, g, 1.0, 4, 64)
    mask = _llama_mask([T, 25], T, dtype)
    bias = torch.randn(1, 4, T, T, generator=g, device=DEV).to(dtype)
    s = ops.attn_matmul(q, k.transpose(2, 3)) / 8.0
    want = ops.attn_matmul(ops.softmax_rows(torch.max((s + bias) + mask, torch.tensor(lo)), torch.float32).to(dtype), v)
    got = ops.attn_fused_clamp(q, k, v, _mul(64), [bias, mask], lo)
    assert torch.equal(_bits(got), _bits(want))
    bias2 = bias.clone()
    bias2[0, 1, 3, 2] = float("nan")                                         # torch.maximum propagates NaN: the row's softmax is NaN
    want = ops.attn_matmul(ops.softmax_rows(torch.max((s + bias2) + mask, torch.tensor(lo)), torch.float32).to(dtype), v)
    got = ops.attn_fused_clamp(q, k, v, _mul(64), [bias2, mask], lo)
    assert bool(torch.isnan(got[0, 1, 3].float()).all()) and torch.equal(torch.isnan(got.float()), torch.isnan(want.float()))
    ok = ~torch.isnan(want.float())
    assert torch.equal(_bits(got)[ok], _bits(want)[ok])


def test_the_entry_point_refuses_what_it_does_not_compute():
    from vlmc import _lib, ops
    dtype = torch.float16
    g = torch.Generator(device=DEV).manual_seed(2)
    q, k, v = _heads(1, 20, dtype, g, 1.0, 2, 64), _heads(1, 20, dtype, g, 1.0, 2, 64), _heads(1, 20, dtype, g, 1.0, 2, 64)
    mask = _llama_mask([20], 20, dtype)
    with pytest.raises(ValueError, match="follows an addend"):
        ops.attn_fused_clamp(q, k, v, None, [], -65504.0)
    for bad in (float("-inf"), float("nan"), -1.00001, -1e30):
        with pytest.raises(_lib.VlmcError, match="finite value of the dtype"):
            ops.attn_fused_clamp(q, k, v, None, [mask], bad)
    # .. and the entry points without a clamp keep their bits next to the new instantiations
    plain = ops.attn_fused(q, k, v, _mul(64), [mask])
    s = ops.attn_matmul(q, k.transpose(2, 3)) / 8.0 + mask
    assert torch.equal(_bits(plain), _bits(ops.attn_matmul(ops.softmax_rows(s, torch.float32).to(dtype), v)))
