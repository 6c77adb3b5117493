"""GPU: `vlmc_attn_fwd_pre` -- the fused attention on the operands as the qkv linear wrote them.  The yardstick is the existing kernel
on operands materialized by torch, the route before: `qkv = y + bias`, the slices of its [B, N, 3, H, d] view, `q * scale`,
`ops.attn_fused`.  Its bits are compared with the new route on the raw `y`: bitwise (`view(torch.int16)`), never a tolerance."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _fp32(v):
    return float(np.float32(v))


def _problem(B, H, N, d, dtype, seed, big_bias=True):
    """y [B, N, 3 H d] with -0.0 entries in its K third; bias = (q_bias, zeros, v_bias), q_bias ~ 8 x |q| so that the add rounds."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = (torch.randn(B, N, 3 * H * d, generator=g, device=DEV) * 0.5).to(dtype)
    y.view(B, N, 3, H, d)[:, ::2, 1, :, ::5] = -0.0
    qb = (torch.randn(H * d, generator=g, device=DEV) * (4.0 if big_bias else 0.5)).to(dtype)
    vb = (torch.randn(H * d, generator=g, device=DEV) * 0.5).to(dtype)
    return y, torch.cat((qb, torch.zeros_like(vb), vb))


def _slices(qkv, B, N, H):
    qkv = qkv.reshape(B, N, 3, H, -1).permute(2, 0, 3, 1, 4)
    return qkv[0], qkv[1], qkv[2]


def _materialized(y, bias, scale, B, N, H, which=("q_add", "k_add", "v_add", "q_mul")):
    """eva_vit.py:133-141 with torch's tensor ops (restricted to the pre-ops in `which`)."""
    C = H * (y.shape[-1] // (3 * H))
    part = torch.zeros_like(bias)
    for i, name in enumerate(("q_add", "k_add", "v_add")):
        if name in which:
            part[i * C:(i + 1) * C] = bias[i * C:(i + 1) * C]
    q, k, v = _slices(y + part if any(n in which for n in ("q_add", "k_add", "v_add")) else y, B, N, H)
    if "q_mul" in which:
        q = q * scale
    return q, k, v


def _pre_kw(bias, scale, H, d, which):
    C = H * d
    kw = {name: bias[i * C:(i + 1) * C].view(H, d) for i, name in enumerate(("q_add", "k_add", "v_add")) if name in which}
    if "q_mul" in which:
        kw["q_mul"] = _fp32(scale)
    return kw


def _score_addend(H, N, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(1, H, N, N, generator=g, device=DEV) * 0.7).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [88, 64])
@pytest.mark.parametrize("n_add", [0, 1])
def test_all_pre_ops_on_packed_and_separate_operands(dtype, d, n_add):
    """B = 2, H = 2, N = 33 (a partial 16-query block, a partial 32-key step, an odd key-tile count); d = 88 is zero-filled to 96."""
    from vlmc import ops
    B, H, N = 2, 2, 33
    scale = d ** -0.5
    y, bias = _problem(B, H, N, d, dtype, 100 + d + n_add)
    adds = [_score_addend(H, N, dtype, 7)] if n_add else []
    want = ops.attn_fused(*_materialized(y, bias, scale, B, N, H), None, adds)
    q, k, v = _slices(y, B, N, H)                                          # strided slices of the packed tensor
    kw = _pre_kw(bias, scale, H, d, ("q_add", "k_add", "v_add", "q_mul"))
    assert _same(ops.attn_fused(q, k, v, None, adds, **kw), want)
    assert _same(ops.attn_fused(q.contiguous(), k.contiguous(), v.contiguous(), None, adds, **kw), want)      # separate tensors (K / V rows 16-byte aligned)
    # the K third of the bias is all zeros and IS applied: -0.0 + 0.0 = +0.0, as `qkv + bias` gives it
    k_mat = _materialized(y, bias, scale, B, N, H)[1]
    assert bool(((_bits(k) == -32768) & (_bits(k_mat) == 0)).any())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [("q_add",), ("k_add",), ("v_add",), ("q_mul",), ("q_add", "q_mul"), ("k_add", "v_add")])
def test_each_pre_op_alone(dtype, which):
    from vlmc import ops
    B, H, N, d = 2, 2, 33, 88
    scale = d ** -0.5
    y, bias = _problem(B, H, N, d, dtype, 300 + len(which))
    want = ops.attn_fused(*_materialized(y, bias, scale, B, N, H, which))
    assert _same(ops.attn_fused(*_slices(y, B, N, H), **_pre_kw(bias, scale, H, d, which)), want)


def test_vit_tile_budget_257_tokens():
    """N = 257 with B = 1, H = 1: 17 query blocks on 8 waves, 18 key tiles."""
    from vlmc import ops
    B, H, N, d, dtype = 1, 1, 257, 88, torch.float16
    scale = d ** -0.5
    y, bias = _problem(B, H, N, d, dtype, 41)
    for adds in ([], [_score_addend(H, N, dtype, 9)]):
        want = ops.attn_fused(*_materialized(y, bias, scale, B, N, H), None, adds)
        assert _same(ops.attn_fused(*_slices(y, B, N, H), None, adds, **_pre_kw(bias, scale, H, d, ("q_add", "k_add", "v_add", "q_mul"))), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_with_lengths_of_a_padded_group(dtype):
    """q_len / k_len 33 / 20 / 1 against the lens route on materialized operands."""
    from vlmc import ops
    B, H, N, d = 3, 2, 33, 64
    scale = d ** -0.5
    y, bias = _problem(B, H, N, d, dtype, 55)
    lens = torch.tensor([33, 20, 1], dtype=torch.int32, device=DEV)
    mask = torch.zeros(B, 1, 1, N, dtype=dtype, device=DEV)
    for j, t in enumerate(lens.tolist()):
        mask[j, :, :, t:] = torch.finfo(dtype).min
    kw = _pre_kw(bias, scale, H, d, ("q_add", "k_add", "v_add", "q_mul"))
    want = ops.attn_fused(*_materialized(y, bias, scale, B, N, H), None, [mask], None, lens, lens)
    assert _same(ops.attn_fused(*_slices(y, B, N, H), None, [mask], None, lens, lens, **kw), want)
    want = ops.attn_fused(*_materialized(y, bias, scale, B, N, H), None, [], None, lens, None)
    assert _same(ops.attn_fused(*_slices(y, B, N, H), None, [], None, lens, None, **kw), want)


def _call_pre(q, k, v, out, *, add0=None, add1=None, has_clamp=0, q_add=None, q_add_ptr=None, has_q_mul=0, q_mul=0.0):
    from vlmc import _lib, ops
    B, H, T, d = q.shape
    I3, I4 = ctypes.c_int64 * 3, ctypes.c_int64 * 4

    def st4(t):
        return None if t is None else I4(*(0 if n == 1 else s for n, s in zip(t.shape[:3], t.stride()[:3])), t.stride(3))
    qa = q_add_ptr if q_add_ptr is not None else (None if q_add is None else q_add.data_ptr())
    return _lib.load().vlmc_attn_fwd_pre(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _lib.F16, B, H, T, k.shape[2], d, I3(*q.stride()[:3]),
                                         I3(*k.stride()[:3]), I3(*v.stride()[:3]), 0, 0.0, None if add0 is None else add0.data_ptr(), st4(add0),
                                         None if add1 is None else add1.data_ptr(), st4(add1), has_clamp, 0.0, None, None, qa,
                                         0 if q_add is None else q_add.stride(0), None, 0, None, 0, has_q_mul, q_mul, ops._stream())


def test_no_pre_op_is_vlmc_attn_fwd_and_refusals():
    from vlmc import _lib, ops
    B, H, N, d = 2, 2, 33, 88
    y, bias = _problem(B, H, N, d, torch.float16, 77)
    q, k, v = _slices(y, B, N, H)
    out = torch.empty(B, N, H, d, dtype=torch.float16, device=DEV)
    assert _call_pre(q, k, v, out) == _lib.VLMC_OK                           # every pre-op null: the bits of vlmc_attn_fwd
    assert _same(out.permute(0, 2, 1, 3), ops.attn_fused(q, k, v))
    qa = bias[:H * d].view(H, d)
    add = _score_addend(H, N, torch.float16, 3)
    assert _call_pre(q, k, v, out, add0=add, q_add=qa) == _lib.VLMC_OK
    assert _call_pre(q, k, v, out, add0=add, has_clamp=1, q_add=qa) == _lib.VLMC_EINVAL            # the clamp variant takes no pre-ops
    assert _call_pre(q, k, v, out, add0=add, add1=add, q_add=qa) == _lib.VLMC_EINVAL               # two score addends
    assert _call_pre(q, k, v, out, q_add=qa, q_add_ptr=qa.data_ptr() + 1) == _lib.VLMC_EINVAL      # a misaligned addend
    assert _call_pre(q, k, v, out, has_q_mul=1, q_mul=float("inf")) == _lib.VLMC_EINVAL            # a non-finite multiplier
    assert _call_pre(q, k, v, out, has_q_mul=1, q_mul=float("nan")) == _lib.VLMC_EINVAL
    torch.cuda.synchronize()
    with pytest.raises(TypeError):
        ops.attn_fused(q, k, v, q_add=qa.float())
    with pytest.raises(ValueError):
        ops.attn_fused(q, k, v, None, [add, add], q_add=qa)


def _eva(dtype=torch.float16):
    from vlmc import synthetic as S
    torch.manual_seed(0)
    mod = S.EvaAttentionOps(176, 2).to(DEV).to(dtype).eval()
    S.randomize_(mod, seed=5)
    g = torch.Generator(device=DEV).manual_seed(6)
    with torch.no_grad():
        mod.q_bias.copy_((torch.randn(176, generator=g, device=DEV) * 2).to(dtype))
        mod.v_bias.copy_((torch.randn(176, generator=g, device=DEV) * 0.5).to(dtype))
    x = (torch.randn(2, 33, 176, generator=g, device=DEV) * 0.5).to(dtype)
    rel = (torch.randn(1, 2, 33, 33, generator=g, device=DEV) * 0.5).to(dtype)
    return mod, x, rel


def test_stand_in_eva_attention_under_the_replay(monkeypatch):
    """dim 176, 2 heads, 33 tokens: `VLMC_ATTN_PRE` 1 and 0 give equal bits, and only 1 moves `stats["attn_fused_pre"]`."""
    from vlmc import forward
    mod, x, rel = _eva()
    linears = [mod.qkv, mod.proj]

    def run():
        with torch.no_grad(), forward.invariant_linears(linears, roots=[mod]):
            return [mod(x), mod(x, rel_pos_bias=rel), mod(x)]
    monkeypatch.setattr(forward, "_FUSED_OK", {})
    monkeypatch.setenv("VLMC_ATTN_PRE", "0")
    before = dict(forward.stats)
    plain = run()
    assert forward.stats["attn_fused_pre"] == before["attn_fused_pre"] and forward.stats["attn_fused"] - before["attn_fused"] == 3
    monkeypatch.setenv("VLMC_ATTN_PRE", "1")
    before = dict(forward.stats)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        pre = run()
    assert forward.stats["attn_fused_pre"] - before["attn_fused_pre"] == 3 and forward.stats["attn_fused"] - before["attn_fused"] == 3
    for a, b in zip(plain, pre):
        assert type(b) is torch.Tensor and _same(a, b)
    assert not any(z._pending() for z in forward._OPERAND_LIVE)


def test_first_use_mismatch_falls_back_with_a_warning(monkeypatch):
    from vlmc import forward, ops
    mod, x, _ = _eva()
    monkeypatch.setenv("VLMC_ATTN_PRE", "0")
    with torch.no_grad(), forward.invariant_linears([mod.qkv, mod.proj], roots=[mod]):
        want = mod(x)
    monkeypatch.setenv("VLMC_ATTN_PRE", "1")
    monkeypatch.setattr(forward, "_FUSED_OK", {})
    real = ops.attn_fused

    def flipped(q, k, v, *a, **kw):
        out = real(q, k, v, *a, **kw)
        if "q_add" in kw:
            out.view(torch.int16)[0, 0, 0, 0] ^= 1
        return out
    monkeypatch.setattr(ops, "attn_fused", flipped)
    before = forward.stats["attn_fused_pre"]
    with torch.no_grad(), forward.invariant_linears([mod.qkv, mod.proj], roots=[mod]):
        with pytest.warns(RuntimeWarning, match="operand pre-ops"):
            got = mod(x)
        again = mod(x)
    assert _same(got, want) and _same(again, want) and forward.stats["attn_fused_pre"] == before
    assert any(v is False for v in forward._FUSED_OK.values())
