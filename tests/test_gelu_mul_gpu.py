"""GPU: `vlmc_gelu_mul` -- T5 v1.1's gated product `F.gelu(wi_0(h)) * wi_1(h)` in one pass.  The yardstick is what the replay ran
before: `ops.gelu(x) * y` (`vlmc_gelu`, then torch's 16-bit `mul`).  Every comparison is bitwise (`view(torch.int16)`), never a tolerance."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
FORMS = ["none", "tanh"]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _y(shape, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * 1.5).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("approximate", FORMS)
def test_every_input_value_times_a_seeded_factor(dtype, approximate):
    """All 65 536 values of x (NaN and infinities included), and the same bits through the element-by-element path of unaligned pointers."""
    from vlmc import ops
    x = torch.arange(65536, dtype=torch.int32, device=DEV).to(torch.int16).view(dtype)
    y = _y((65536,), dtype, 5)
    want = ops.gelu(x, approximate) * y
    got = ops.gelu_mul(x, y, approximate)
    assert _same(got, want), f"{int((_bits(got) != _bits(want)).sum())} of 65536 products differ from gelu(x) * y"
    # 2 bytes off a 16-byte boundary: x alone, y alone, both
    pad = torch.zeros(65537, dtype=dtype, device=DEV)
    xo, yo = pad.clone(), pad.clone()
    xo[1:], yo[1:] = x, y
    assert xo[1:].data_ptr() % 16 == 2
    for a, b in ((xo[1:], y), (x, yo[1:]), (xo[1:], yo[1:])):
        assert _same(ops.gelu_mul(a, b, approximate), want)
    for n in (1, 7, 8, 9, 4097):                               # any length, any position
        assert _same(ops.gelu_mul(x[:n], y[:n], approximate), want[:n])
        assert _same(ops.gelu_mul(x[65536 - n:], y[65536 - n:], approximate), want[65536 - n:])


@pytest.mark.parametrize("dtype", DTYPES)
def test_odd_widths_and_pitched_column_slices(dtype):
    """[7, 2048 + 609] (a last partial block in torch's kernels, a pitch that rules the 16-byte path out), the same width at a pitch
    that allows it (a row's last partial step), and the two outputs of one grouped launch as column slices of one buffer."""
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(17)
    rows, cols = 7, 2048 + 609
    x = (torch.randn(rows, cols, generator=g, device=DEV) * 2).to(dtype)
    y = _y((rows, cols), dtype, 18)
    for approximate in FORMS:
        want = ops.gelu(x, approximate) * y
        assert _same(ops.gelu_mul(x, y, approximate), want)
        buf = torch.zeros(rows, 2 * 2664 + 8, dtype=dtype, device=DEV)             # pitch 5336 = 8 * 667
        xs, ys = buf[:, :cols], buf[:, 2664:2664 + cols]
        xs.copy_(x)
        ys.copy_(y)
        assert xs.data_ptr() % 16 == 0 and ys.data_ptr() % 16 == 0 and not xs.is_contiguous()
        assert _same(ops.gelu_mul(xs, ys, approximate), want)
        assert _same(ops.gelu_mul(xs, y, approximate), want) and _same(ops.gelu_mul(x, ys, approximate), want)
    for cols, pitch in ((40, 88), (44, 96), (160, 320)):                              # 16-byte path / y 8 bytes off / wi_0 | wi_1 of d_ff 160
        buf = (torch.randn(3, 11, pitch, generator=g, device=DEV) * 2).to(dtype)
        xs, ys = buf[..., :cols], buf[..., cols:2 * cols]
        got = ops.gelu_mul(xs, ys)
        assert got.shape == (3, 11, cols) and got.is_contiguous()
        assert _same(got, ops.gelu(xs.contiguous()) * ys)


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_map_computes_real_rows_only(dtype):
    """3 samples x 7 padded tokens x 40 columns, lengths 7 / 3 / 0: NaN / Inf in the padding rows of x and y reach nothing, the padding
    rows of the product are exactly zero, and a sample's rows have the bits they have alone."""
    from vlmc import ops
    lengths, P, cols = [7, 3, 0], 7, 40
    n = len(lengths)
    g = torch.Generator(device=DEV).manual_seed(23)
    x = (torch.randn(n, P, cols, generator=g, device=DEV) * 2).to(dtype)
    y = _y((n, P, cols), dtype, 24)
    tok = np.arange(P)[None, :]
    real = tok < np.asarray(lengths)[:, None]
    flat = np.arange(n)[:, None] * P + tok
    rowmap = torch.from_numpy(np.concatenate([flat[real], flat[~real]]).astype(np.int32)).to(DEV)
    n_real = int(real.sum())
    xp, yp = x.clone(), y.clone()
    for j, t in enumerate(lengths):
        xp[j, t:, 0::3], xp[j, t:, 1::3], xp[j, t:, 2::3] = float("nan"), float("inf"), float("-inf")
        yp[j, t:, 0::2], yp[j, t:, 1::2] = float("inf"), float("nan")
    for approximate in FORMS:
        dense = ops.gelu(x, approximate) * y
        got = ops.gelu_mul(xp, yp, approximate, rowmap, n_real)
        assert got.shape == x.shape
        for j, t in enumerate(lengths):
            assert _same(got[j, :t], dense[j, :t])
            assert bool((_bits(got[j, t:]) == 0).all()), "a padding row of the product is not +0"
            if t:
                assert _same(ops.gelu_mul(x[j:j + 1, :t], y[j:j + 1, :t], approximate), got[j:j + 1, :t])      # alone == inside the group
    with pytest.raises(ValueError):
        ops.gelu_mul(x, y, "none", rowmap[:-1], n_real)
    with pytest.raises(TypeError):
        ops.gelu_mul(x, y.float())
    with pytest.raises(TypeError):
        ops.gelu_mul(x, y[:, :, :8])


def test_entry_point_refuses_bad_arguments():
    from vlmc import _lib, ops
    lib = _lib.load()
    x = torch.zeros(4, 16, dtype=torch.float16, device=DEV)
    out = torch.empty_like(x)
    s = ops._stream()
    call = lambda *a: lib.vlmc_gelu_mul(*a, s)
    assert call(x.data_ptr(), x.data_ptr(), out.data_ptr(), _lib.F16, 0, 4, 16, 16, 16, 16, None, 0) == _lib.VLMC_OK
    assert call(x.data_ptr(), x.data_ptr(), out.data_ptr(), _lib.F32, 0, 4, 16, 16, 16, 16, None, 0) == _lib.VLMC_EINVAL
    assert call(x.data_ptr(), x.data_ptr(), out.data_ptr(), _lib.F16, 2, 4, 16, 16, 16, 16, None, 0) == _lib.VLMC_EINVAL
    assert call(x.data_ptr(), x.data_ptr(), out.data_ptr(), _lib.F16, 0, 4, 16, 8, 16, 16, None, 0) == _lib.VLMC_EINVAL       # pitch < cols
    assert call(x.data_ptr() + 1, x.data_ptr(), out.data_ptr(), _lib.F16, 0, 3, 16, 16, 16, 16, None, 0) == _lib.VLMC_EINVAL  # odd address
    assert call(None, x.data_ptr(), out.data_ptr(), _lib.F16, 0, 4, 16, 16, 16, 16, None, 0) == _lib.VLMC_EINVAL
    rm = torch.arange(4, dtype=torch.int32, device=DEV)
    assert call(x.data_ptr(), x.data_ptr(), out.data_ptr(), _lib.F16, 0, 4, 16, 16, 16, 16, rm.data_ptr(), 5) == _lib.VLMC_EINVAL
    torch.cuda.synchronize()


def _ffn(blk, x):
    """The feed-forward third of the stand-in T5 block (vlmc/synthetic.py: T5Block.forward; modeling_t5.py:337-346)."""
    ff = blk.layer[-1]
    d = ff.DenseReluDense
    h = ff.layer_norm(x)
    return x + d.wo(F.gelu(d.wi_0(h)) * d.wi_1(h))


@pytest.mark.parametrize("padded", [False, True])
def test_stand_in_t5_ffn_keeps_its_bits(padded, monkeypatch):
    """dim 64, d_ff 160 under the replay's patches: `VLMC_GELU_MUL` 1 and 0 give equal bits, dense and inside a padded group; the lazy
    GELU exists only for outputs of a sibling-group launch and only with the switch on."""
    from vlmc import forward
    from vlmc import synthetic as S
    torch.manual_seed(0)
    blk = S.T5Block(64, 160, 2, 32, False).to(DEV).bfloat16().eval()
    S.randomize_(blk, seed=3)
    d = blk.layer[-1].DenseReluDense
    linears = [d.wi_0, d.wi_1, d.wo]
    lengths, P = [7, 3, 5], 7
    n = len(lengths)
    g = torch.Generator(device=DEV).manual_seed(31)
    x = (torch.randn(n, P, 64, generator=g, device=DEV) * 0.5).bfloat16()
    maps = None
    if padded:
        tok = np.arange(P)[None, :]
        real = tok < np.asarray(lengths)[:, None]
        flat = np.arange(n)[:, None] * P + tok
        for j, t in enumerate(lengths):
            x[j, t:] = 0
        maps = {(n, P): (torch.from_numpy(np.concatenate([flat[real], flat[~real]]).astype(np.int32)).to(DEV), int(real.sum()))}

    def run():
        with torch.no_grad(), forward.invariant_linears(linears, roots=[blk]), forward.padded_rows(maps):
            return [_ffn(blk, x) for _ in range(3)]                        # (the first forward learns that wi_0 / wi_1 are siblings)
    monkeypatch.setattr(forward, "_GELU_MUL_OK", {})
    monkeypatch.setenv("VLMC_GELU_MUL", "0")
    before = dict(forward.stats)
    two_ops = run()
    assert forward.stats["gelu_mul"] == before["gelu_mul"] and forward.stats["gelu_kernel"] - before["gelu_kernel"] == 3
    monkeypatch.setenv("VLMC_GELU_MUL", "1")
    before = dict(forward.stats)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                     # (the first-use comparison warns when the bits differ)
        fused = run()
    assert forward.stats["gelu_mul"] - before["gelu_mul"] == 3 and forward.stats["gelu_mul_checks"] - before["gelu_mul_checks"] == 1
    assert forward.stats["grouped_launches"] - before["grouped_launches"] == 3
    assert all(v for v in forward._GELU_MUL_OK.values()) and len(forward._GELU_MUL_OK) == 1
    for a, b in zip(two_ops, fused):
        assert type(b) is torch.Tensor and _same(a, b)
    if padded:
        for j, t in enumerate(lengths):
            assert bool((fused[-1][j, t:] == 0).all())
    # a GELU whose argument is no sibling output (ViT's gelu(fc1(..))) is computed at once, as before
    with torch.no_grad(), forward.invariant_linears(linears, roots=[blk]):
        assert type(F.gelu(d.wo(torch.zeros(2, 160, dtype=torch.bfloat16, device=DEV)))) is torch.Tensor

