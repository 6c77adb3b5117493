"""The compiled host path (csrc/fastpath/fast_bind.cpp -> vlmc/_fast) and the ctypes back end (vlmc/ops.py: _ctypes_route) call the same
C ABI under one contract: same bits, same refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _both(monkeypatch, fn):
    from vlmc import ops
    assert ops._fast is not None, "vlmc/_fast is not built (python -c 'import __graft_entry__ as g; g.build()')"
    fast = fn()
    monkeypatch.setattr(ops, "_fast", None)
    slow = fn()
    monkeypatch.undo()
    return fast, slow


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_linear_routes_agree(dtype, monkeypatch):
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(3, 37, 256, generator=g, device=DEV).to(dtype)
    ws = [torch.randn(n, 256, generator=g, device=DEV).to(dtype) for n in (64, 200, 96)]
    bs = [torch.randn(64, generator=g, device=DEV).to(dtype), None, torch.randn(96, generator=g, device=DEV).to(dtype)]
    for w, b in zip(ws, bs):
        a, c = _both(monkeypatch, lambda: ops.linear_fwd(x, w, b))
        assert a.shape == (3, 37, w.shape[0]) and torch.equal(a, c)
    a, c = _both(monkeypatch, lambda: ops.linear_fwd_group(x, ws, bs))
    assert len(a) == 3 and all(torch.equal(p, q) for p, q in zip(a, c))
    assert all(torch.equal(p, ops.linear_fwd(x, w, b)) for p, w, b in zip(a, ws, bs))
    # a strided input (column slice of a wider buffer) and an expanded one
    wide = torch.randn(37, 512, generator=g, device=DEV).to(dtype)
    a, c = _both(monkeypatch, lambda: ops.linear_fwd(wide[:, 256:], ws[0], bs[0]))
    assert torch.equal(a, c) and torch.equal(a, ops.linear_fwd(wide[:, 256:].contiguous(), ws[0], bs[0]))
    row = torch.randn(1, 256, generator=g, device=DEV).to(dtype).expand(5, 256)
    a, c = _both(monkeypatch, lambda: ops.linear_fwd(row, ws[1]))
    assert torch.equal(a, c)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_row_mapped_linear_routes_agree(dtype, monkeypatch):
    """vlmc_linear_fwd_rows through vlmc/_fast and through ctypes: same outputs (16-bit group launch; fp32 one launch per member), and
    a call the kernel does not take raises what the public op says."""
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(3)
    lengths, tp, K = [9, 3, 12, 1, 7], 12, 256
    x = (torch.randn(len(lengths), tp, K, generator=g, device=DEV) * 0.5).to(dtype)
    real = [j * tp + t for j, n in enumerate(lengths) for t in range(n)]
    pad = [j * tp + t for j, n in enumerate(lengths) for t in range(n, tp)]
    rowmap = torch.tensor(real + pad, dtype=torch.int32, device=DEV)
    ws = [(torch.randn(n, K, generator=g, device=DEV) * 0.05).to(dtype) for n in (64, 200)]
    bs = [(torch.randn(64, generator=g, device=DEV) * 0.1).to(dtype), None]
    a, c = _both(monkeypatch, lambda: ops.linear_fwd_rows(x, ws, bs, rowmap, len(real)))
    assert len(a) == 2 and all(p.shape == (len(lengths), tp, w.shape[0]) and torch.equal(p, q) for p, q, w in zip(a, c, ws))
    with pytest.raises(ValueError):
        ops.linear_fwd_rows(x, ws, bs, rowmap[:-1].contiguous(), len(real))          # (the back end answers None, the public op says why)


def test_attention_products_routes_agree(monkeypatch):
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(1)
    qkv = (torch.randn(2, 33, 3 * 4 * 88, generator=g, device=DEV) * 0.5).half().reshape(2, 33, 3, 4, 88).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    a, c = _both(monkeypatch, lambda: ops.attn_matmul(q, k.transpose(-2, -1)))
    assert torch.equal(a, c)
    p = a.softmax(-1)
    a, c = _both(monkeypatch, lambda: ops.attn_matmul(p, v))
    assert torch.equal(a, c)
    a, c = _both(monkeypatch, lambda: ops.attn_matmul(p[0], v[0]))                     # 3-D
    assert torch.equal(a, c) and a.shape == (4, 33, 88)
    a, c = _both(monkeypatch, lambda: ops.attn_matmul(p[:1], v))                       # broadcast batch
    assert torch.equal(a, c) and a.shape == (2, 4, 33, 88)


def test_both_routes_refuse_the_same_calls(monkeypatch):
    from vlmc import ops
    x = torch.randn(4, 64, device=DEV)
    w = torch.randn(8, 64, device=DEV)
    for fast in (True, False):
        if not fast:
            monkeypatch.setattr(ops, "_fast", None)
        assert ops.linear_fwd(x, w).dtype == torch.float32               # fp32: taken since round 6 (the fp32 kernel, both routes)
        with pytest.raises(TypeError):
            ops.linear_fwd(x.double(), w.double())                       # fp64
        with pytest.raises(TypeError):
            ops.linear_fwd(x.half(), w)                                  # mixed dtypes
        assert ops.linear_fwd(x.half(), w, _try=True) is None
        with pytest.raises(TypeError):
            ops.linear_fwd_group(x.half(), [w.half(), w])                # mixed dtypes
        with pytest.raises(ValueError):
            ops.linear_fwd_group(x.half(), [w.half()] * 5)               # more than 4 members
        with pytest.raises(TypeError):
            ops.attn_matmul(x.half()[None], w.half().t()[None].float())
        with pytest.raises(RuntimeError):
            ops.linear_fwd(x.cpu().half(), w.cpu().half())               # no CPU fallback on either route


def test_sdpa_and_rms_norm_routes_agree(monkeypatch):
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(3)
    qkv = torch.randn(3, 70, 3 * 8 * 64, generator=g, device=DEV).to(torch.bfloat16)
    q, k, v = (t.reshape(3, 70, 8, 64).transpose(1, 2) for t in qkv.reshape(3, 70, 3, 8 * 64).unbind(2))
    a, c = _both(monkeypatch, lambda: ops.sdpa(q, k, v))
    assert a.shape == (3, 8, 70, 64) and torch.equal(a, c) and a.stride() == c.stride()
    a, c = _both(monkeypatch, lambda: ops.sdpa(q[:, :, :16], k, v, scale=0.2))
    assert torch.equal(a, c)
    a, c = _both(monkeypatch, lambda: ops.sdpa(q, k, v, causal=True))
    assert torch.equal(a, c) and not torch.equal(a, ops.sdpa(q, k, v))
    big = torch.randn(1, 2, 8, 300, 64, generator=g, device=DEV).to(torch.float16)       # more keys than a head may have
    a, c = _both(monkeypatch, lambda: ops.sdpa(big[0, :, :, :8], big[0], big[0], _try=True))
    assert a is None and c is None
    for fn in (lambda: ops.sdpa(q.float(), k.float(), v.float()), lambda: ops.sdpa(q, k, v, scale=-1.0)):
        for route in (True, False):
            if not route:
                monkeypatch.setattr(ops, "_fast", None)
            with pytest.raises(TypeError):
                fn()
            monkeypatch.undo()
    x = torch.randn(4, 9, 520, generator=g, device=DEV).to(torch.float16)
    w = (torch.randn(520, generator=g, device=DEV) * 0.2 + 1).to(torch.float16)
    a, c = _both(monkeypatch, lambda: ops.rms_norm(x, w, 1e-6, 0))
    assert a.shape == x.shape and torch.equal(a, c)
    a, c = _both(monkeypatch, lambda: ops.rms_norm(x[:, :, :], w, 1e-5, 1))
    assert torch.equal(a, c)
    for route in (True, False):
        if not route:
            monkeypatch.setattr(ops, "_fast", None)
        with pytest.raises(TypeError):
            ops.rms_norm(x, w.float(), 1e-6, 0)
        monkeypatch.undo()


def _each_route(monkeypatch):
    """The compiled route, then the ctypes one (`ops._fast` is looked up per call)."""
    from vlmc import ops
    assert ops._fast is not None, "vlmc/_fast is not built (python -c 'import __graft_entry__ as g; g.build()')"
    yield "compiled"
    monkeypatch.setattr(ops, "_fast", None)
    yield "ctypes"
    monkeypatch.undo()


def test_fp32_launches_routes_agree(monkeypatch):
    """The fp32 kernels behind linear_fwd and attn_matmul through both routes: the loose rows view (`ld = K` for a single row) and the
    one attn_matmul launch of the ctypes back end."""
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(4, 64, generator=g, device=DEV)
    w = torch.randn(8, 64, generator=g, device=DEV)
    b = torch.randn(8, generator=g, device=DEV)
    for bias in (None, b):
        a, c = _both(monkeypatch, lambda: ops.linear_fwd(x, w, bias))
        assert a.dtype == torch.float32 and a.shape == (4, 8) and torch.equal(a, c)
    wide = torch.randn(1, 200, generator=g, device=DEV)
    row = wide[:, 70:134]                                                # M = 1, a column slice: stride(0) = 200, the kernel is told ld = K
    a, c = _both(monkeypatch, lambda: ops.linear_fwd(row, w, b))
    assert a.shape == (1, 8) and torch.equal(a, c) and torch.equal(a, ops.linear_fwd(row.contiguous(), w, b))
    p = torch.randn(2, 3, 9, 16, generator=g, device=DEV)
    q = torch.randn(2, 3, 16, 9, generator=g, device=DEV)
    a, c = _both(monkeypatch, lambda: ops.attn_matmul(p, q))
    assert a.dtype == torch.float32 and a.shape == (2, 3, 9, 9) and torch.equal(a, c)
    a, c = _both(monkeypatch, lambda: ops.attn_matmul(p[1], q[1]))       # 3-D
    assert a.shape == (3, 9, 9) and torch.equal(a, c) and torch.equal(a, ops.attn_matmul(p, q)[1])


def test_row_mean_routes_agree(monkeypatch):
    from vlmc import ops
    x = torch.randn(5, 7, 300, generator=torch.Generator(device=DEV).manual_seed(6), device=DEV)
    for keepdim in (False, True):
        a, c = _both(monkeypatch, lambda: ops.row_mean(x, keepdim))
        assert a.shape == ((5, 7, 1) if keepdim else (5, 7)) and torch.equal(a, c)
        a, c = _both(monkeypatch, lambda: ops.row_mean(x[:, :, :257], keepdim))          # rows 300 apart, read in place
        assert torch.equal(a, c) and torch.equal(a, ops.row_mean(x[:, :, :257].contiguous(), keepdim))
        a, c = _both(monkeypatch, lambda: ops.row_mean(x[2, 3:4, :257], keepdim))        # a single row
        assert a.shape == ((1, 1) if keepdim else (1,)) and torch.equal(a, c)
        assert torch.equal(a.reshape(-1), ops.row_mean(x[:, :, :257])[2, 3:4])


def test_row_mapped_linear_refusals_on_both_routes(monkeypatch):
    from vlmc import ops
    x = torch.randn(2, 6, 64, device=DEV).half()
    w = torch.randn(8, 64, device=DEV).half()
    rowmap = torch.arange(12, dtype=torch.int32, device=DEV)
    for route in _each_route(monkeypatch):
        with pytest.raises(ValueError):
            ops.linear_fwd_rows(x, [w], [None], rowmap[:-1].contiguous(), 5)             # a short row map
        with pytest.raises(ValueError):
            ops.linear_fwd_rows(x, [w] * 5, None, rowmap, 5)                             # more than 4 members
        with pytest.raises(TypeError):
            ops.linear_fwd_rows(x, [w, w.float()], None, rowmap, 5)                      # mixed dtypes
        with pytest.raises(RuntimeError):
            ops.linear_fwd_rows(x.cpu(), [w], [None], rowmap, 5)                         # no CPU fallback
        with pytest.raises(RuntimeError):
            ops.linear_fwd_rows(x, [w], [None], rowmap.cpu(), 5)


def test_every_op_refuses_alike_on_both_routes(monkeypatch):
    """One refused call or more for each of the seven ops: the same exception class on both routes, None under `_try`.  Every one is
    refused by the host checks, before any launch."""
    from vlmc import ops
    x = torch.randn(4, 64, device=DEV)
    w = torch.randn(8, 64, device=DEV)
    xh, wh = x.half(), w.half()
    rowmap = torch.arange(4, dtype=torch.int32, device=DEV)
    q = torch.randn(1, 2, 5, 16, device=DEV).half()
    refused = [                      # (op, arguments, keyword arguments, exception class)
        ("linear_fwd", (xh, w), {}, TypeError),                                          # mixed dtypes
        ("linear_fwd", (xh[:, :60], wh[:, :60]), {}, TypeError),                         # in_features % 8
        ("linear_fwd", (x, w, torch.zeros(8, device=DEV).half()), {}, TypeError),        # fp32 with a 16-bit bias
        ("linear_fwd", (xh.cpu(), wh.cpu()), {}, RuntimeError),
        ("linear_fwd_group", (xh, [wh, w]), {}, TypeError),
        ("linear_fwd_group", (x, [w]), {}, TypeError),                                   # fp32: not a group launch
        ("linear_fwd_group", (xh, []), {}, ValueError),
        ("linear_fwd_group", (xh, [wh] * 2, [None]), {}, ValueError),                    # fewer biases than weights
        ("linear_fwd_group", (xh.cpu(), [wh.cpu()] * 5), {}, RuntimeError),
        ("linear_fwd_rows", (xh, [wh], [None], rowmap, 0), {}, ValueError),              # n_real < 1
        ("linear_fwd_rows", (xh, [wh], [None], rowmap.long(), 4), {}, ValueError),
        ("linear_fwd_rows", (x, [w, wh], None, rowmap, 4), {}, TypeError),
        ("attn_matmul", (xh, wh.t()), {}, TypeError),                                    # 2-D
        ("attn_matmul", (xh[None], w.t()[None]), {}, TypeError),                         # mixed dtypes
        ("attn_matmul", (xh[None].cpu(), wh.t()[None].cpu()), {}, RuntimeError),
        ("rms_norm", (xh, torch.ones(64, device=DEV), 1e-6), {}, TypeError),             # an fp32 weight
        ("rms_norm", (x, torch.ones(64, device=DEV), 1e-6), {}, TypeError),              # fp32 x
        ("rms_norm", (xh, torch.ones(64).half(), 1e-6), {}, RuntimeError),               # a CPU weight
        ("sdpa", (q.float(), q.float(), q.float()), {}, TypeError),
        ("sdpa", (q, q, q), {"scale": 0.0}, TypeError),
        ("sdpa", (q, q[:, :, :, :8], q), {}, TypeError),                                 # head_dim of k
        ("sdpa", (q.cpu(), q.cpu(), q.cpu()), {}, RuntimeError),
        ("row_mean", (xh,), {}, TypeError),
        ("row_mean", (x[:, :0],), {}, TypeError),                                        # empty rows
        ("row_mean", (x.cpu(),), {}, RuntimeError),
    ]
    assert {op for op, *_ in refused} == set(ops._FAST_ENTRY_POINTS)
    for route in _each_route(monkeypatch):
        for op, args, kw, exc in refused:
            with pytest.raises(exc) as info:
                getattr(ops, op)(*args, **kw)
            assert type(info.value) is exc and (exc is RuntimeError or f"vlmc.{op}: " in str(info.value)), (route, op, info.value)
            if op in ("linear_fwd", "attn_matmul", "sdpa"):
                assert getattr(ops, op)(*args, _try=True, **kw) is None, (route, op)
