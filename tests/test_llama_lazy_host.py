"""CPU: the clamp of the reference's LLaMA attention (modeling_llama.py:235-236) in the lazy attention chain of `vlmc/forward.py`, with
the kernels replaced by torch stand-ins (as tests/test_attn_lazy_host.py does for the other chains) -- every accepted spelling is
recorded and reaches the clamp entry point with `clamp_min`; a bound the kernel cannot take, or a clamp in another place, is
computed from the literal record; a chain without a clamp calls `ops.attn_fused` exactly as before.  And `plan_padded`: `position_ids`
is a kwarg it knows how to pad, an unknown tensor kwarg still is not."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from vlmc import forward, ops


_MATMUL, _SOFTMAX, _MAXIMUM = torch.matmul, torch.softmax, torch.maximum


def _mm(a, b, *_a, **_k):
    return _MATMUL(a.float(), b.float()).to(a.dtype)


def _softmax_rows(x, out_dtype=None):
    return _SOFTMAX(x.float(), -1).to(x.dtype if out_dtype is None else out_dtype)


class _Fused:
    """stands in for ops.attn_fused / ops.attn_fused_clamp: the chain, op by op, from the arguments the fused kernel would get"""
    def __init__(self):
        self.calls = []

    def _run(self, q, k, v, mul, adds, clamp):
        s = _mm(q, k.transpose(-1, -2))
        if mul is not None:
            s = (s.float() * torch.tensor(mul, dtype=torch.float32)).to(q.dtype)
        for t in adds:
            s = (s.float() + t.float()).to(q.dtype)
        if clamp is not None:
            s = _MAXIMUM(s, torch.tensor(clamp, dtype=q.dtype))
        p = _SOFTMAX(s.float(), -1).to(q.dtype)
        return _mm(p, v).transpose(1, 2).contiguous().transpose(1, 2)

    def plain(self, q, k, v, mul=None, adds=(), _plan=None):               # (today's signature, as tests/test_attn_lazy_host.py has it)
        self.calls.append({"mul": mul, "adds": list(adds), "clamp": None})
        return self._run(q, k, v, mul, adds, None)

    def clamp(self, q, k, v, mul=None, adds=(), clamp_min=0.0, _plan=None, q_len=None, k_len=None):
        self.calls.append({"mul": mul, "adds": list(adds), "clamp": clamp_min, "q_len": q_len, "k_len": k_len})
        return self._run(q, k, v, mul, adds, clamp_min)


@pytest.fixture
def fake_kernels(monkeypatch):
    n_threads = torch.get_num_threads()
    torch.set_num_threads(1)
    fused = _Fused()
    monkeypatch.setattr(ops, "attn_matmul", lambda a, b, _plan=None, _try=False: _mm(a, b))
    monkeypatch.setattr(ops, "attn_fused_plan", functools.partial(ops.attn_fused_plan, _cuda_only=False))
    monkeypatch.setattr(ops, "attn_fused", fused.plain)
    monkeypatch.setattr(ops, "attn_fused_clamp", fused.clamp)
    monkeypatch.setattr(ops, "softmax_rows", _softmax_rows)
    monkeypatch.setattr(ops, "_need_gpu", lambda *a: None)
    monkeypatch.setattr(ops, "_attn_max_keys", {8: 512, 16: 512})
    monkeypatch.setattr(forward, "_FUSED_OK", {})
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    yield fused
    torch.set_num_threads(n_threads)


def _qkv(B=2, H=3, T=6, d=8, dtype=torch.float16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, T, H, d, generator=g).to(dtype).transpose(1, 2) for _ in range(3))


def _mask(B, T, dtype):
    """causal + right padding of the last sample, both at the dtype's minimum and ADDED (modeling_llama.py:470-491): -inf where both hide"""
    lo = torch.finfo(dtype).min
    causal = torch.full((T, T), lo).triu(1).to(dtype)[None, None].expand(B, 1, T, T)
    pad = torch.zeros(B, 1, T, T, dtype=dtype)
    pad[-1, :, :, T - 2:] = lo
    m = pad + causal
    assert torch.isinf(m).any() and m.dtype == dtype
    return m


def _llama(q, k, v, mask, clamp):                                             # modeling_llama.py:222-240
    w = torch.matmul(q, k.transpose(2, 3)) / math.sqrt(q.shape[-1])
    w = w + mask
    w = clamp(w)
    w = F.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
    return torch.matmul(w, v)


def _run(fn, *a):
    with torch.no_grad(), forward.invariant_matmuls():
        return fn(*a)


SPELLINGS = {
    "torch.max(x, t)": lambda dt: (lambda w: torch.max(w, torch.tensor(torch.finfo(dt).min))),      # the reference's
    "torch.maximum": lambda dt: (lambda w: torch.maximum(w, torch.tensor(torch.finfo(dt).min))),
    "Tensor.max(t)": lambda dt: (lambda w: w.max(torch.tensor(torch.finfo(dt).min))),
    "Tensor.maximum": lambda dt: (lambda w: w.maximum(torch.tensor(torch.finfo(dt).min, dtype=dt))),
    "clamp(min=number)": lambda dt: (lambda w: w.clamp(min=torch.finfo(dt).min)),
    "torch.clamp(min=tensor)": lambda dt: (lambda w: torch.clamp(w, min=torch.tensor(torch.finfo(dt).min))),
    "clamp_min": lambda dt: (lambda w: w.clamp_min(torch.finfo(dt).min)),
    "torch.clamp_min": lambda dt: (lambda w: torch.clamp_min(w, torch.finfo(dt).min)),
}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("spelling", sorted(SPELLINGS))
def test_the_clamp_is_recorded_in_every_spelling_and_reaches_the_clamp_entry_point(fake_kernels, spelling, dtype):
    q, k, v = _qkv(dtype=dtype)
    mask = _mask(2, 6, dtype)
    clamp = SPELLINGS[spelling](dtype)
    want = _llama(q, k, v, mask, clamp)                                    # plain torch
    seen = {}

    def probe(w):
        r = clamp(w)
        seen["in"], seen["out"] = type(w), type(r)
        seen["clamp"] = getattr(r, "_clamp", "realized")
        return r
    before = dict(forward.stats)
    got = _run(_llama, q, k, v, mask, probe)
    assert seen["in"] is forward.LazyScores and seen["out"] is forward.LazyScores, f"{spelling}: the chain was realized at the clamp"
    assert seen["clamp"] == torch.finfo(dtype).min
    c = fake_kernels.calls[-1]
    import numpy as np
    assert c["clamp"] == torch.finfo(dtype).min and c["mul"] == float(np.float32(1) / np.float32(math.sqrt(8))) and \
        len(c["adds"]) == 1 and c["adds"][0] is mask
    assert forward.stats["attn_fused"] == before["attn_fused"] + 1 and forward.stats["attn_fused_clamp"] == before["attn_fused_clamp"] + 1
    assert forward.stats["attn_fused_checks"] == before["attn_fused_checks"] + 1      # a new signature: compared with the unfused ops once
    assert torch.isfinite(got.float()).all()
    assert torch.allclose(got.float(), want.float(), atol=2e-2)
    got2 = _run(_llama, q, k, v, mask, clamp)
    assert forward.stats["attn_fused_checks"] == before["attn_fused_checks"] + 1
    assert forward.stats["attn_chain_unfused"] == before["attn_chain_unfused"] + 1
    assert torch.equal(got, got2)


def test_the_realized_clamped_chain_has_the_values_of_the_plain_ops(fake_kernels, monkeypatch):
    """VLMC_ATTN_CLAMP=0 (the cross-check route): the clamp realizes the chain; -inf entries of the mask come out clamped either way"""
    q, k, v = _qkv()
    mask = _mask(2, 6, torch.float16)
    clamp = SPELLINGS["torch.max(x, t)"](torch.float16)
    fused = _run(_llama, q, k, v, mask, clamp)
    monkeypatch.setenv("VLMC_ATTN_CLAMP", "0")
    n = len(fake_kernels.calls)
    types_ = []

    def probe(w):
        r = clamp(w)
        types_.append(type(r))
        return r
    unfused = _run(_llama, q, k, v, mask, probe)
    assert types_ == [torch.Tensor] and len(fake_kernels.calls) == n
    assert torch.equal(fused, unfused)


@pytest.mark.parametrize("case", ["non_scalar", "requires_grad", "before_the_addend", "not_a_value_of_the_dtype", "infinite", "upper_bound",
                                  "reduction"])
def test_a_bound_the_kernel_cannot_take_realizes_the_chain(fake_kernels, case):
    q, k, v = _qkv()
    mask = _mask(2, 6, torch.float16)
    lo = torch.finfo(torch.float16).min
    out_types = []

    def chain(q, k, v, plain):
        mm = _mm if plain else torch.matmul
        w = mm(q, k.transpose(2, 3)) / math.sqrt(q.shape[-1])
        if case == "before_the_addend":
            w = torch.max(w, torch.tensor(lo))
            out_types.append(type(w))
            w = w + mask
        else:
            w = w + mask
            if case == "non_scalar":
                w = torch.max(w, torch.full((6,), lo, dtype=torch.float16))
            elif case == "requires_grad":
                w = torch.max(w, torch.tensor(lo, requires_grad=True)).detach()
            elif case == "not_a_value_of_the_dtype":
                w = torch.max(w, torch.tensor(-1.00001))                       # (fp16 has no such value)
            elif case == "infinite":
                w = torch.max(w, torch.tensor(float("-inf")))
            elif case == "upper_bound":
                w = torch.clamp(w, min=lo, max=3.0)
            elif case == "reduction":
                w = torch.max(w, -1, keepdim=True)[0].expand(2, 3, 6, 6).contiguous()      # torch.max(x, int): a reduction, not the clamp
            out_types.append(type(w))
        w = (_softmax_rows(w, torch.float32) if plain else F.softmax(w, dim=-1, dtype=torch.float32)).to(q.dtype)
        return mm(w, v)
    n = len(fake_kernels.calls)
    with torch.no_grad():
        want = chain(q, k, v, True)
    out_types.clear()
    got = _run(chain, q, k, v, False)
    assert out_types == [torch.Tensor], f"{case}: not realized"
    assert len(fake_kernels.calls) == n                                     # neither fused entry point
    assert torch.equal(got, want)


def test_a_chain_without_a_clamp_calls_attn_fused_with_todays_arguments(fake_kernels):
    q, k, v = _qkv()
    mask = torch.zeros(2, 1, 1, 6, dtype=torch.float16)

    def qformer(q, k, v):
        s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
        return torch.matmul(torch.softmax(s + mask, -1), v)
    _run(qformer, q, k, v)
    assert fake_kernels.calls[-1]["clamp"] is None                          # `_Fused.plain` takes (q, k, v, mul, adds, _plan) and nothing else


# ---- plan_padded ----------------------------------------------------------------------------------------------------------------
def _caches(lengths, extra=None, dtype=torch.float16):
    xs, cs = [], []
    for t in lengths:
        xs.append(torch.zeros(1, t, 16, dtype=dtype))
        m = torch.full((t, t), torch.finfo(dtype).min, dtype=dtype).triu(1)[None, None]
        c = {"attention_mask": m, "position_ids": torch.arange(t)[None]}
        if extra is not None:
            c.update(extra(t))
        cs.append(c)
    return xs, cs


@pytest.fixture
def host_padding(monkeypatch):
    """replay_padding with `plan_padded` runnable on the host: it asks for CUDA inputs (only while it plans) and builds its row maps
    through a pinned staging buffer"""
    import types
    from lavis.compression.pruners import replay_padding as rp
    monkeypatch.setattr(rp, "int32_on", lambda values, device: torch.as_tensor(values, dtype=torch.int32))

    def plan_padded(*a):
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
            return rp.plan_padded(*a)
    return types.SimpleNamespace(plan_padded=plan_padded, _pad_caches=rp._pad_caches)


def test_plan_padded_forms_one_group_for_ragged_llama_caches(host_padding):
    rp = host_padding
    lengths = [5, 9, 7, 9, 3]
    xs, cs = _caches(lengths)
    plan = rp.plan_padded(xs, cs, len(xs), 128)
    assert plan is not None and len(plan) == 1, "ragged samples with position_ids must form ONE padded group"
    chunk, spec = plan[0]
    assert chunk == list(range(5)) and spec["tp"] == 9 and spec["T"] == lengths
    kw = rp._pad_caches(cs, spec)
    pos = kw["position_ids"]
    assert pos.shape == (5, 9) and pos.dtype == torch.int64
    for j, t in enumerate(lengths):
        assert torch.equal(pos[j, :t], torch.arange(t)) and not pos[j, t:].any()       # 0 behind a sample's tokens
    m = kw["attention_mask"]
    lo = torch.finfo(torch.float16).min
    assert m.shape == (5, 1, 9, 9)
    for j, t in enumerate(lengths):
        assert torch.equal(m[j, :, :t, :t], cs[j]["attention_mask"][0]) and (m[j, :, :t, t:] == lo).all()


def test_plan_padded_still_refuses_what_it_does_not_know(host_padding):
    rp = host_padding
    xs, cs = _caches([5, 9, 7], extra=lambda t: {"cache_position": torch.arange(t)[None]})
    assert rp.plan_padded(xs, cs, 3, 128) is None                           # a tensor kwarg nobody told it how to pad
    xs, cs = _caches([5, 9, 7])
    cs[1]["position_ids"] = cs[1]["position_ids"].float()
    cs[0]["position_ids"], cs[2]["position_ids"] = cs[0]["position_ids"].float(), cs[2]["position_ids"].float()
    assert rp.plan_padded(xs, cs, 3, 128) is None                           # positions that are not integers
    xs, cs = _caches([5, 9, 7])
    cs[2]["position_ids"] = torch.arange(6)[None]
    assert rp.plan_padded(xs, cs, 3, 128) is None                           # .. or not one per token
    xs, cs = _caches([6, 6, 6])
    assert rp.plan_padded(xs, cs, 3, 128) is None                           # not ragged: groups of equal shape
