"""GPU: the TILED packed linear (vlmc_linear_fwd_24_tiled / _48_tiled, `ops.linear_fwd_24(.., tiled=True)` / `ops.linear_fwd_48`): the
register-staged GEMM with its weight operand packed n:m gives, bit for bit and in every tile shape, what the dense batch-invariant
kernel gives on the unpacked weight, at any number of rows and without a scratch weight.  No tolerance anywhere: every comparison
is on int16 views."""
import functools

import pytest
import torch

import variant_runs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
FORMATS = ["24", "48"]
NM = {"24": (2, 4), "48": (4, 8)}

# every tile shape of launch_gemm: the rule's own pick, the four forced shapes, and 256 x 256 from one tile on
VARIANTS = {"default": {}, "128": {"VLMC_GEMM_SHAPE": "128"}, "64": {"VLMC_GEMM_SHAPE": "64"}, "p32": {"VLMC_GEMM_SHAPE": "p32"},
            "32": {"VLMC_GEMM_SHAPE": "32"}, "256": {"VLMC_GEMM_BIG_TILES": "1"}}
# N below a panel of every shape, a half panel (136 against 128), more than one panel; K below one tile of 64, a tail of one chunk
# (72), several tiles; M below, at and just past the tile edges, and a multiple of none
SWEEP_N, SWEEP_K, SWEEP_M = (1, 17, 33, 136, 300), (8, 40, 64, 72, 200, 1408), (1, 65, 127, 129, 300)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _op(fmt, name):
    from vlmc import ops
    return getattr(ops, f"{name}_{fmt}")


def _pruned(fmt, n, k, dtype, gen, scale=0.05):
    """(values, meta, dense W . mask, mask) of a random weight pruned 2:4 or 4:8 by the n:m rule"""
    from vlmc import ops
    W = (torch.randn(n, k, generator=gen, device=DEV) * scale).to(dtype)
    sq = torch.rand(k, generator=gen, device=DEV) + 0.5
    keep, _ = ops.wanda_select(W, sq, "nm", n=NM[fmt][0], m=NM[fmt][1])
    values, meta = _op(fmt, "pack")(W, keep)
    dense, k2 = _op(fmt, "unpack")(values, meta)
    assert torch.equal(k2, keep) and _same(dense, W)
    return values, meta, dense, keep


@functools.lru_cache(maxsize=None)
def _case(fmt, n, k, dtype):
    """one pruned weight, bias and 300 rows of activations per (format, N, K, dtype): the same in every process, never written to"""
    gen = torch.Generator(device=DEV).manual_seed(100000 * int(fmt) + 1000 * n + k)
    values, meta, dense, keep = _pruned(fmt, n, k, dtype, gen)
    bias = torch.randn(n, generator=gen, device=DEV).to(dtype)
    x = torch.randn(300, k, generator=gen, device=DEV).to(dtype)
    return values, meta, dense, keep, bias, x


def _sweep(run):
    """{key: run(fmt, x, values, meta, dense, bias)} over the whole sweep, on the CPU"""
    out = {}
    for fmt in FORMATS:
        for dtype in DTYPES:
            for n in SWEEP_N:
                for k in SWEEP_K:
                    values, meta, dense, _keep, bias, x = _case(fmt, n, k, dtype)
                    for m in SWEEP_M:
                        for b in (None, bias):
                            key = f"{fmt}/{str(dtype)[6:]}/n{n}/k{k}/m{m}/{'bias' if b is not None else 'nobias'}"
                            out[key] = run(fmt, x[:m], values, meta, dense, b).cpu()
    return out


def tiled_sweep():
    """(child process, one per tile-shape variant) the tiled kernel over the sweep"""
    return _sweep(lambda fmt, x, values, meta, dense, b: _op(fmt, "linear_fwd")(x, values, meta, b, tiled=True))


def test_every_tile_shape_both_formats_both_dtypes(tmp_path):
    from vlmc import ops
    results = variant_runs.run_variants(tmp_path, "test_linear_nm_tiled_gpu", "tiled_sweep", VARIANTS)
    assert len(results["default"]) == 2 * 2 * len(SWEEP_N) * len(SWEEP_K) * len(SWEEP_M) * 2
    variant_runs.assert_variants_agree(results)
    want = _sweep(lambda fmt, x, values, meta, dense, b: ops.linear_fwd(x, _op(fmt, "unpack")(values, meta)[0], b))
    variant_runs.assert_variants_agree({"default": want, "tiled": results["default"]})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_routes_agree(fmt, dtype):
    from vlmc import ops
    fwd = _op(fmt, "linear_fwd")
    for n, k in ((33, 1408), (300, 200)):
        values, meta, dense, _keep, bias, x = _case(fmt, n, k, dtype)
        for m in (1, 64, 65, 300):
            want = ops.linear_fwd(x[:m], dense, bias)
            assert _same(fwd(x[:m], values, meta, bias, tiled=True), want), (n, k, m)
            assert _same(fwd(x[:m], values, meta, bias, unpack=True), want), (n, k, m)
            assert _same(fwd(x[:m], values, meta, bias), want), (n, k, m)
            assert _same(fwd(x[:m], values, meta, bias, tiled=False), want), (n, k, m)
    with pytest.raises(ValueError):
        fwd(x, values, meta, bias, unpack=True, tiled=True)
    assert ops.linear_fwd_24_tiled_max_rows() == 0 or ops.linear_fwd_24_tiled_max_rows() >= ops.linear_fwd_24_max_rows()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_rows_do_not_depend_on_the_batch(fmt, dtype):
    fwd = _op(fmt, "linear_fwd")
    values, meta, _dense, _keep, bias, x = _case(fmt, 33, 1408, dtype)
    big = fwd(x, values, meta, bias, tiled=True)
    small = fwd(x[:65], values, meta, bias, tiled=True)
    for i in (0, 64, 299):
        alone = fwd(x[i:i + 1], values, meta, bias)                            # M = 1: the carried-chain kernel
        assert _same(big[i:i + 1], alone), i
        if i < 65:
            assert _same(small[i:i + 1], alone), i
    # the same row at another place of a 65-row call
    assert _same(fwd(x[235:300], values, meta, bias, tiled=True)[64:65], big[299:300])
    # leading dims
    assert _same(fwd(x[:12].reshape(3, 4, -1), values, meta, bias, tiled=True).reshape(12, -1), big[:12])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_strided_rows_and_an_offset_start(fmt, dtype):
    """ldx > K, ldy > N and X starting 16 bytes into its allocation, through the C entry point, at M = 65"""
    from vlmc import _lib, ops
    n, k, m = 33, 40, 65
    values, meta, dense, _keep, bias, x = _case(fmt, n, k, dtype)
    ldx, ldy = k + 16, n + 3
    xbuf = torch.zeros(8 + m * ldx, dtype=dtype, device=DEV)
    xs = xbuf[8:].view(m, ldx)
    xs[:, :k] = x[:m]
    xs[:, k:] = float("nan")                                                  # never read
    assert xs.data_ptr() % 16 == 0 and xs.data_ptr() == xbuf.data_ptr() + 16
    y = torch.full((m, ldy), 7.0, dtype=dtype, device=DEV)
    entry = getattr(_lib.load(), f"vlmc_linear_fwd_{fmt}_tiled")
    _lib.check(entry(xs.data_ptr(), values.data_ptr(), meta.data_ptr(), bias.data_ptr(), ops._DT[dtype], m, n, k, ldx, y.data_ptr(), ldy,
                     ops._stream()))
    want = ops.linear_fwd(x[:m], dense, bias)
    assert not bool(torch.isnan(want).any())
    assert _same(y[:, :n], want)
    assert bool((y[:, n:] == 7.0).all())                                      # nothing written past a row's N outputs
    # the same rows as a strided view, through the wrapper
    assert _same(_op(fmt, "linear_fwd")(xs[:, :k], values, meta, bias, tiled=True), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_kept_zeros_and_an_inf_at_a_pruned_column(fmt, dtype):
    from vlmc import ops
    fwd = _op(fmt, "linear_fwd")
    n, k, m = 17, 64, 65
    gen = torch.Generator(device=DEV).manual_seed(5)
    W = (torch.randn(n, k, generator=gen, device=DEV) * 0.05).to(dtype)
    keep, _ = ops.wanda_select(W, torch.ones(k, device=DEV), "nm", n=NM[fmt][0], m=NM[fmt][1])
    # a kept +0 and a kept -0: positions come from the mask, the values travel as they are
    c0, c1 = (int(c) for c in keep[3].nonzero().flatten()[:2])
    W[3, c0], W[3, c1] = 0.0, -0.0
    values, meta = _op(fmt, "pack")(W, keep)
    dense, k2 = _op(fmt, "unpack")(values, meta)
    assert torch.equal(k2, keep) and int(_bits(dense)[3, c1]) == -32768
    x = torch.randn(m, k, generator=gen, device=DEV).to(dtype)
    assert _same(fwd(x, values, meta, tiled=True), ops.linear_fwd(x, dense))
    # rows of X that meet the kept -0 alone (+1 and -1 at its column, +0 elsewhere): the dense kernel's signs of zero
    xz = torch.zeros(m, k, dtype=dtype, device=DEV)
    xz[0, c1], xz[1, c1] = 1.0, -1.0
    assert _same(fwd(xz, values, meta, tiled=True), ops.linear_fwd(xz, dense))
    # inf in X at a column that row 5's mask prunes (and other rows keep): the dense layer multiplies inf by the stored zero
    col = int((~keep[5]).nonzero().flatten()[0])
    xi = x.clone()
    xi[2, col] = float("inf")
    got, want = fwd(xi, values, meta, tiled=True), ops.linear_fwd(xi, dense)
    assert bool(torch.isnan(want[2, 5])) and not bool(torch.isnan(want[3]).any())
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert torch.equal(_bits(got)[ok], _bits(want)[ok])


@pytest.mark.parametrize("fmt,n,k,dtype", [("24", 11008, 4096, torch.float16), ("24", 4096, 11008, torch.float16),
                                           ("48", 6144, 1408, torch.bfloat16)])
def test_model_widths_at_257_rows(fmt, n, k, dtype):
    from vlmc import ops
    gen = torch.Generator(device=DEV).manual_seed(n)
    values, meta, dense, _keep = _pruned(fmt, n, k, dtype, gen, scale=0.02)
    x = torch.randn(257, k, generator=gen, device=DEV).to(dtype)
    assert _same(_op(fmt, "linear_fwd")(x, values, meta, tiled=True), ops.linear_fwd(x, dense))


def no_scratch_child():
    """(child process: the shared scratch weight of the unpack route is empty) peak allocation of one tiled forward at 4096 x 4096"""
    from vlmc import ops
    from vlmc.packed24 import Linear24
    n = k = 4096
    gen = torch.Generator(device=DEV).manual_seed(9)
    values, meta, dense, _keep = _pruned("24", n, k, torch.float16, gen, scale=0.02)
    lin = Linear24(values, meta)
    x = torch.randn(257, k, generator=gen, device=DEV).half()
    want = ops.linear_fwd(x, dense)
    del dense, _keep
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    y = ops.linear_fwd_24(x, lin.weight_packed24, lin.weight_meta24, lin.bias, tiled=True)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    return {"grown": grown, "same": _same(y, want), "finite": bool(torch.isfinite(want).all())}


def test_no_scratch_weight(tmp_path):
    r = variant_runs.run_variants(tmp_path, "test_linear_nm_tiled_gpu", "no_scratch_child", {"default": {}})["default"]
    assert r["grown"] < 4096 * 4096 * 2, r["grown"]
    assert r["same"] and r["finite"]


# ---- a packed model ------------------------------------------------------------------------------------------------------------
def _toy_2_4():
    """the 16-bit toy InstructBLIP (fp16 ViT, bf16 T5) pruned 2:4 by the drop-in Wanda pruner, and one batch"""
    from lavis.compression import load_pruner
    import toy_models
    model = toy_models.init_toy(toy_models.ToyBlipT5(vit_dtype=torch.float16, t5_dtype=torch.bfloat16), seed=7).eval().to(DEV)
    batches = [{k: t.to(DEV) for k, t in b.items()} for b in toy_models.make_batches(4, seed=11)]
    spec = "2-0.5-1.0-1.0"
    cfg = dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method="wanda", vit_pruning_method="wanda", num_samples=4,
               prune_n=2, prune_m=4, max_sparsity_per_layer=1.01)
    pruned, _ = load_pruner("blipt5_wanda_pruner", model, batches, cfg=cfg).prune()
    return pruned, batches[0]


def _invariant_forward(model, batch):
    """one forward with every plain linear on ops.linear_fwd"""
    from vlmc import forward
    import torch.nn as nn
    linears = [m for m in model.modules() if type(m) is nn.Linear]
    with torch.no_grad(), forward.invariant_linears(linears):
        return model(batch)["logits"]


def test_packed_toy_model_with_every_linear_tiled(monkeypatch):
    from vlmc import ops
    from vlmc.packed24 import Linear24, pack_model_24_
    pruned, batch = _toy_2_4()
    want = _invariant_forward(pruned, batch)
    assert want.dtype == torch.float32 and bool(torch.isfinite(want).all())
    names = pack_model_24_(pruned)
    assert len(names) == 2 * 4 + 2 * 7 + 2 * 11 and all(isinstance(pruned.get_submodule(n), Linear24) for n in names)
    plain, calls = ops.linear_fwd_24, []

    def forced(x, values, meta, bias=None):
        calls.append(x.numel() // x.shape[-1])
        return plain(x, values, meta, bias, tiled=True)

    monkeypatch.setattr(ops, "linear_fwd_24", forced)
    got = _invariant_forward(pruned, batch)
    assert len(calls) >= len(names)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
