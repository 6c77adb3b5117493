"""CPU: the lazy operands of `vlmc/forward.py` -- `LazyGelu` (the gated product) and `LazyOperand` (a qkv linear's output that the
model biases, slices and scales) -- with the kernels replaced by torch stand-ins: what reaches the fused entry points, and that anything
else is computed by the model's own torch ops (the model's code sees the values it would have seen)."""
import pytest
import torch
import torch.nn.functional as F

from vlmc import _lib, forward, ops

_GELU = F.gelu                                                            # the original (the stand-ins may run under the patches)


class _GeluMul:
    """stands in for ops.gelu_mul: the two ops, from the arguments the kernel would get"""
    def __init__(self):
        self.calls = []
        self.flip = False

    def __call__(self, x, y, approximate="none", rowmap=None, n_real=0):
        self.calls.append({"x": x, "y": y, "approximate": approximate, "rowmap": rowmap, "n_real": n_real})
        out = _GELU(x, approximate=approximate) * y
        if rowmap is not None:
            out.view(-1, out.shape[-1])[rowmap[n_real:].long()] = 0
        if self.flip:
            out.view(torch.int16)[..., 0] ^= 1
        return out


@pytest.fixture
def fake_kernels(monkeypatch):
    fused = _GeluMul()
    monkeypatch.setattr(ops, "gelu", lambda x, approximate="none": _GELU(x, approximate=approximate))
    monkeypatch.setattr(ops, "gelu_mul", fused)
    monkeypatch.setattr(forward, "_GELU_MUL_OK", {})
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return fused


def _xy(shape=(3, 5, 16), dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype), torch.randn(shape, generator=g).to(dtype)


@pytest.mark.parametrize("approximate", ["none", "tanh"])
@pytest.mark.parametrize("spell", [lambda a, b: a * b, lambda a, b: a.mul(b), torch.mul])
def test_the_gated_product_reaches_the_one_pass_kernel(fake_kernels, approximate, spell):
    x, y = _xy()
    before = dict(forward.stats)
    with torch.no_grad():
        z = forward.LazyGelu(x, approximate)
        assert z.shape == x.shape and z.dtype == x.dtype and z.dim() == 3 and z.size(-1) == 16 and not fake_kernels.calls
        out = spell(z, y)
        again = spell(forward.LazyGelu(x, approximate), y)
    assert type(out) is torch.Tensor and torch.equal(out, _GELU(x, approximate=approximate) * y) and torch.equal(again, out)
    assert len(fake_kernels.calls) == 2 and fake_kernels.calls[0]["x"] is x and fake_kernels.calls[0]["y"] is y
    assert fake_kernels.calls[0]["approximate"] == approximate and fake_kernels.calls[0]["rowmap"] is None
    assert forward.stats["gelu_mul"] - before["gelu_mul"] == 2 and forward.stats["gelu_mul_checks"] - before["gelu_mul_checks"] == 1
    assert forward.stats["gelu_kernel"] - before["gelu_kernel"] == 1        # (the first-use comparison ran the two ops once)


def test_the_row_map_of_the_argument_goes_along(fake_kernels):
    x, y = _xy((2, 4, 8))
    rowmap = torch.tensor([0, 1, 2, 4, 3, 5, 6, 7], dtype=torch.int32)
    x.view(-1, 8)[rowmap[4:].long()] = 0                                   # (what vlmc_linear_fwd_rows leaves in the padding rows
    y.view(-1, 8)[rowmap[4:].long()] = 0                                   # of wi_0's and wi_1's outputs alike)
    x._vlmc_rows = (rowmap, 4)
    with torch.no_grad():
        out = forward.LazyGelu(x, "none") * y
    assert fake_kernels.calls[-1]["rowmap"] is rowmap and fake_kernels.calls[-1]["n_real"] == 4
    assert torch.equal(out, _GELU(x) * y) and out._vlmc_rows == (rowmap, 4)


def test_every_other_use_computes_the_gelu_first(fake_kernels):
    x, y = _xy()
    want = _GELU(x)
    before = dict(forward.stats)
    with torch.no_grad():
        for use, ref in ((lambda z: z + y, want + y), (lambda z: torch.relu(z), torch.relu(want)), (lambda z: z.float(), want.float()),
                         (lambda z: y * z, y * want),                                       # (the model's order is gelu * linear)
                         (lambda z: z * 0.5, want * 0.5), (lambda z: z * y[:, :1], want * y[:, :1]), (lambda z: z * y.float(), want * y.float()),
                         (lambda z: torch.mul(z, y, out=torch.empty_like(y)), want * y), (lambda z: z.view(-1, 16), want.view(-1, 16)),
                         (lambda z: F.linear(z, y[0, :4]), F.linear(want, y[0, :4]))):
            z = forward.LazyGelu(x, "none")
            got = use(z)
            assert type(got) is torch.Tensor and torch.equal(got, ref)
            assert z._real is not None and torch.equal(z._real, want)
    assert not fake_kernels.calls and forward.stats["gelu_mul"] == before["gelu_mul"]
    with torch.no_grad():                                                   # realized once: its product is torch's from then on
        z = forward.LazyGelu(x, "none")
        z.sum()
        assert torch.equal(z * y, want * y) and not fake_kernels.calls
    with torch.enable_grad():                                               # gradients enabled: never the kernel
        assert torch.equal(forward.LazyGelu(x, "none") * y, want * y) and not fake_kernels.calls


def test_a_mismatch_at_first_use_keeps_the_two_ops(fake_kernels):
    x, y = _xy()
    fake_kernels.flip = True
    with torch.no_grad():
        with pytest.warns(RuntimeWarning, match="vlmc_gelu_mul does not reproduce"):
            out = forward.LazyGelu(x, "none") * y
        assert torch.equal(out, _GELU(x) * y) and len(fake_kernels.calls) == 1
        assert list(forward._GELU_MUL_OK.values()) == [False]
        before = forward.stats["gelu_mul"]
        assert torch.equal(forward.LazyGelu(x, "none") * y, _GELU(x) * y)
    assert len(fake_kernels.calls) == 1 and forward.stats["gelu_mul"] == before


def test_no_verdict_is_taken_during_a_graph_capture(fake_kernels, monkeypatch):
    x, y = _xy()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with torch.no_grad():
        assert torch.equal(forward.LazyGelu(x, "none") * y, _GELU(x) * y)
    assert not fake_kernels.calls and not forward._GELU_MUL_OK


def test_plain_tensors_get_a_plain_gelu(monkeypatch):
    """The patched `F.gelu` hands out a lazy result for a tagged sibling output only (and never with the switch off)."""
    x, _ = _xy()
    gelu = forward._make_gelu(_GELU)
    monkeypatch.setattr(forward, "_mm_owner", forward._ident())
    with torch.no_grad():
        assert type(gelu(x)) is torch.Tensor                                  # (a CPU tensor: the original)
    assert forward.gelu_mul_enabled()
    monkeypatch.setenv("VLMC_GELU_MUL", "0")
    assert not forward.gelu_mul_enabled()
    monkeypatch.setenv("VLMC_GELU_MUL", "1")
    monkeypatch.setenv("VLMC_GELU", "0")
    assert not forward.gelu_mul_enabled()


def test_the_new_exports_are_declared_and_bound():
    for name in ("vlmc_gelu_mul", "vlmc_attn_fwd_pre"):
        assert name in _lib.header_functions() and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.header_abi_version() >= 28


# ---- LazyOperand -----------------------------------------------------------------------------------------------------------------
B_, N_, H_, D_ = 2, 5, 3, 8


def _qkv(dtype=torch.float16, seed=1):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B_, N_, 3 * H_ * D_, generator=g).to(dtype)
    bias = torch.randn(3 * H_ * D_, generator=g).to(dtype)
    return y, bias


def _eva_slices(t):
    t = t.reshape(B_, N_, 3, H_, -1).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def test_view_ops_keep_addend_and_raw_tensor_aligned():
    y, bias = _qkv()
    scale = D_ ** -0.5
    with torch.no_grad():
        z = forward.LazyOperand(y) + bias
        assert type(z) is forward.LazyOperand and z._raw is y and z._add.shape == y.shape and z._add.stride() == (0, 0, 1)
        want = y + bias
        q, k, v = _eva_slices(z)
        wq, wk, wv = _eva_slices(want)
        q = q * scale
        assert all(type(t) is forward.LazyOperand and t._pending() for t in (q, k, v)) and q._mul == float(torch.tensor(scale, dtype=torch.float32))
        # whatever slice reaches the matmul carries its own slice of the bias, with head and d strides
        for i, t in enumerate((q, k, v)):
            assert t._raw.shape == (B_, H_, N_, D_) and t._raw.data_ptr() == y.data_ptr() + 2 * i * H_ * D_
            assert t._add.stride() == (0, D_, 0, 1) and t._add.data_ptr() == bias.data_ptr() + 2 * i * H_ * D_
            ad = forward._head_addend(t)
            assert ad.shape == (H_, D_) and torch.equal(ad, bias[i * H_ * D_:(i + 1) * H_ * D_].view(H_, D_))
        raw = forward._pre_ops(q, k, v)
        assert raw is not None and sorted(raw[3]) == ["k_add", "q_add", "q_mul", "v_add"] and raw[0] is q._raw
        assert torch.equal(q._realize(), wq * scale) and torch.equal(k._realize(), wk) and torch.equal(v._realize(), wv)
        # the other view ops
        for view in (lambda t: t.transpose(1, 2), lambda t: torch.transpose(t, 0, 2), lambda t: t.view(B_ * N_, -1), lambda t: t.select(2, 7),
                     lambda t: t.narrow(2, 8, 16), lambda t: t[:, 1:3], lambda t: t.unbind(1)[2], lambda t: t.chunk(3, dim=-1)[1],
                     lambda t: torch.reshape(t, (B_, N_, 3, -1)).permute(2, 0, 1, 3)[2]):
            got = view(forward.LazyOperand(y) + bias)
            assert type(got) is forward.LazyOperand and got._raw.shape == got._add.shape == view(want).shape
            assert torch.equal(got._realize(), view(want))


def test_anything_else_realizes_the_operand():
    y, bias = _qkv()
    want = y + bias
    other = torch.randn_like(y)
    with torch.no_grad():
        for use, ref in ((lambda z: torch.relu(z), torch.relu(want)), (lambda z: z.float(), want.float()), (lambda z: z.sum(-1), want.sum(-1)),
                         (lambda z: z + bias, want + bias),                                       # a second addend
                         (lambda z: z * other, want * other),                                     # a tensor multiplier
                         (lambda z: (z * 0.5) * 0.25, (want * 0.5) * 0.25),                       # a second scalar multiply
                         (lambda z: (z * 0.5) + bias, (want * 0.5) + bias),                       # an addend behind a multiply
                         (lambda z: bias + z, bias + want), (lambda z: z - bias, want - bias), (lambda z: z.contiguous(), want),
                         (lambda z: z[torch.tensor([1, 0])], want[torch.tensor([1, 0])]),          # advanced indexing is no view
                         (lambda z: z.transpose(0, 1).reshape(N_ * B_, -1), want.transpose(0, 1).reshape(N_ * B_, -1)),      # a reshape that copies
                         (lambda z: torch.nn.functional.linear(z, other[0, :4]), torch.nn.functional.linear(want, other[0, :4]))):
            got = use(forward.LazyOperand(y) + bias)
            assert type(got) is torch.Tensor and torch.equal(got, ref)
        assert type(forward.LazyOperand(y) + bias.float()) is torch.Tensor                            # another dtype: torch's promotion
        assert type(forward.LazyOperand(y) * 2) is forward.LazyOperand and type(2.0 * forward.LazyOperand(y)) is forward.LazyOperand
    with torch.enable_grad():
        assert type(forward.LazyOperand(y) + bias) is torch.Tensor


def test_nothing_stays_pending_after_realize_escaped():
    y, bias = _qkv()
    with torch.no_grad():
        held = [forward.LazyOperand(y) + bias, _eva_slices(forward.LazyOperand(y) + bias)[0] * 0.5, forward.LazyOperand(y)]
        assert held[0]._pending() and held[1]._pending() and not held[2]._pending()
        forward._realize_escaped()
        assert not any(z._pending() for z in forward._OPERAND_LIVE)
        assert torch.equal(held[0]._real, y + bias) and torch.equal(held[1]._real, _eva_slices(y + bias)[0] * 0.5)


def test_only_a_bias_fed_linear_is_flagged(monkeypatch):
    import torch.nn as nn
    from vlmc import synthetic as S
    eva = S.EvaAttentionOps(16, 2)
    plain = S.Attention(16, 2, 8, fused_qkv=True)                          # a fused qkv linear nobody biases
    blk = nn.ModuleList([eva, plain])
    linears = [eva.qkv, eva.proj, plain.qkv, plain.proj]
    assert forward._bias_fed_linears([blk], linears) == {id(eva.qkv)}
    assert forward._bias_fed_linears([blk], [eva.proj, plain.qkv]) == set()                    # (only linears the replay patches)
    eva.qkv.bias = nn.Parameter(torch.zeros(48))
    assert forward._bias_fed_linears([blk], linears) == set()                                  # a linear with a bias of its own
    tracker = forward._Tracker(linears)
    assert tracker.bias_fed == set()
    assert forward.attn_pre_enabled()
    monkeypatch.setenv("VLMC_ATTN_PRE", "0")
    assert not forward.attn_pre_enabled()
