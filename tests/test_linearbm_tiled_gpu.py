"""GPU: the TILED bitmap-packed linear (vlmc_linear_fwd_bm_tiled, `ops.linear_fwd_bm(.., tiled=True)`): the register-staged GEMM with its
weight operand bitmap-packed gives, bit for bit and in every tile shape, what the dense batch-invariant kernel gives on the unpacked
weight, at any number of rows, under any mask layout and without a scratch weight; whatever the metadata holds it reads nothing outside
`values`.  No tolerance anywhere: every comparison is on int16 views."""
import functools

import pytest
import torch

import variant_runs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]

# every tile shape of launch_gemm: the rule's own pick, the four forced shapes, and 256 x 256 from one tile on
VARIANTS = {"default": {}, "128": {"VLMC_GEMM_SHAPE": "128"}, "64": {"VLMC_GEMM_SHAPE": "64"}, "p32": {"VLMC_GEMM_SHAPE": "p32"},
            "32": {"VLMC_GEMM_SHAPE": "32"}, "256": {"VLMC_GEMM_BIG_TILES": "1"}}
# N below a panel of every shape, a half panel (136 against 128), more than one panel; K = 8 and 40 put every row's meta at an odd byte
# offset and end in the last-dword clamp, 72 and 200 leave a K tail, 40 and 200 a partial last offs step, 1408 several tiles; M below,
# at and just past the tile edges, and a multiple of none
SWEEP_N, SWEEP_K, SWEEP_M = (1, 17, 33, 136, 300), (8, 40, 64, 72, 200, 1408), (1, 65, 127, 129, 300)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _masked(W, keep):
    """W . mask with +0 at the pruned positions (a product would leave -0 under a negative weight)"""
    return torch.where(keep, W, torch.zeros_like(W))


def _pack(W, keep):
    """(packed = (values, meta, offs, rowptr), dense W . mask) -- the round trip checked"""
    from vlmc import ops
    packed = ops.pack_bm(W, keep)
    dense, k2 = ops.unpack_bm(*packed)
    assert torch.equal(k2, keep) and _same(dense, _masked(W, keep))
    return packed, dense


@functools.lru_cache(maxsize=None)
def _case(n, k, dtype):
    """one weight under a random mask of density 0.5, bias and 300 rows of activations per (N, K, dtype): the same in every process,
    never written to"""
    gen = torch.Generator(device=DEV).manual_seed(77000000 + 1000 * n + k)
    W = (torch.randn(n, k, generator=gen, device=DEV) * 0.05).to(dtype)
    keep = torch.rand(n, k, generator=gen, device=DEV) < 0.5
    packed, dense = _pack(W, keep)
    bias = torch.randn(n, generator=gen, device=DEV).to(dtype)
    x = torch.randn(300, k, generator=gen, device=DEV).to(dtype)
    return packed, dense, keep, bias, x


def _sweep(run):
    """{key: run(x, packed, dense, bias)} over the whole sweep, on the CPU"""
    out = {}
    for dtype in DTYPES:
        for n in SWEEP_N:
            for k in SWEEP_K:
                packed, dense, _keep, bias, x = _case(n, k, dtype)
                for m in SWEEP_M:
                    for b in (None, bias):
                        key = f"{str(dtype)[6:]}/n{n}/k{k}/m{m}/{'bias' if b is not None else 'nobias'}"
                        out[key] = run(x[:m], packed, dense, b).cpu()
    return out


def tiled_sweep():
    """(child process, one per tile-shape variant) the tiled kernel over the sweep"""
    from vlmc import ops
    return _sweep(lambda x, packed, dense, b: ops.linear_fwd_bm(x, *packed, b, tiled=True))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
def test_every_tile_shape_both_dtypes(tmp_path):
    from vlmc import ops
    results = variant_runs.run_variants(tmp_path, "test_linearbm_tiled_gpu", "tiled_sweep", VARIANTS)
    assert len(results["default"]) == 2 * len(SWEEP_N) * len(SWEEP_K) * len(SWEEP_M) * 2
    variant_runs.assert_variants_agree(results)
    want = _sweep(lambda x, packed, dense, b: ops.linear_fwd(x, ops.unpack_bm(*packed)[0], b))
    variant_runs.assert_variants_agree({"default": want, "tiled": results["default"]})


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
LAYOUTS = ["density_0.05", "density_0.5", "density_0.95", "density_1.0", "all_false", "empty_first_and_last", "odd_rowptr", "one_column_per_row",
           "full_and_empty_rows"]


def _layout(name, n, k, gen):
    keep = torch.rand(n, k, generator=gen, device=DEV) < 0.5
    if name.startswith("density_"):
        d = float(name[8:])
        keep = torch.rand(n, k, generator=gen, device=DEV) < d if d < 1.0 else torch.ones(n, k, dtype=torch.bool, device=DEV)
    elif name == "all_false":
        keep[:] = False
    elif name == "empty_first_and_last":
        keep[0] = False
        keep[n - 1] = False
    elif name == "odd_rowptr":
        # row 0 keeps one column, every later row an even number: every row after the first starts at an odd index
        keep[0] = False
        keep[0, 3] = True
        odd = keep[1:].sum(1) % 2 == 1
        keep[1:, 0] ^= odd
    elif name == "one_column_per_row":
        # the last position of a chunk, another chunk in every row: one set bit per row, bit 7 of its byte
        keep[:] = False
        rows = torch.arange(n, device=DEV)
        keep[rows, 8 * (rows % (k // 8)) + 7] = True
    elif name == "full_and_empty_rows":
        keep[:] = False
        keep[0::2] = True
    return keep


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_mask_layouts(layout, dtype):
    from vlmc import ops
    for n, k in ((33, 1408), (300, 200)):
        gen = torch.Generator(device=DEV).manual_seed(6 + n)
        W = (torch.randn(n, k, generator=gen, device=DEV) * 0.05).to(dtype)
        keep = _layout(layout, n, k, gen)
        packed, dense = _pack(W, keep)
        meta, rowptr = packed[1], packed[3].cpu()
        if layout == "density_1.0":
            assert bool((meta == 255).all()) and int(rowptr[n]) == n * k
        elif layout == "all_false":
            assert int(rowptr[n]) == 0 and packed[0].numel() == 16
        elif layout == "empty_first_and_last":
            assert int(rowptr[0]) == int(rowptr[1]) == 0 and int(rowptr[n - 1]) == int(rowptr[n])
        elif layout == "odd_rowptr":
            assert bool((rowptr[1:] % 2 == 1).all())
        elif layout == "one_column_per_row":
            assert int(rowptr[n]) == n and bool(((meta == 0) | (meta == 128)).all())
        x = torch.randn(129, k, generator=gen, device=DEV).to(dtype)
        bias = torch.randn(n, generator=gen, device=DEV).to(dtype)
        assert _same(ops.linear_fwd_bm(x, *packed, bias, tiled=True), ops.linear_fwd(x, dense, bias)), (n, k)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_routes_agree(dtype):
    from vlmc import ops
    for n, k in ((33, 1408), (300, 200)):
        packed, dense, _keep, bias, x = _case(n, k, dtype)
        for m in (1, 16, 17, 64, 65, 300):
            want = ops.linear_fwd(x[:m], dense, bias)
            assert _same(ops.linear_fwd_bm(x[:m], *packed, bias, tiled=True), want), (n, k, m)
            assert _same(ops.linear_fwd_bm(x[:m], *packed, bias, unpack=True), want), (n, k, m)
            assert _same(ops.linear_fwd_bm(x[:m], *packed, bias), want), (n, k, m)
            assert _same(ops.linear_fwd_bm(x[:m], *packed, bias, tiled=False), want), (n, k, m)
    with pytest.raises(ValueError):
        ops.linear_fwd_bm(x, *packed, bias, unpack=True, tiled=True)
    assert ops.linear_fwd_bm_tiled_max_rows() == 0 or ops.linear_fwd_bm_tiled_max_rows() >= ops.linear_fwd_bm_max_rows()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_do_not_depend_on_the_batch(dtype):
    from vlmc import ops
    packed, _dense, _keep, bias, x = _case(33, 1408, dtype)
    big = ops.linear_fwd_bm(x, *packed, bias, tiled=True)
    small = ops.linear_fwd_bm(x[:65], *packed, bias, tiled=True)
    for i in (0, 64, 299):
        alone = ops.linear_fwd_bm(x[i:i + 1], *packed, bias, tiled=False)      # M = 1: the carried-chain kernel
        assert _same(big[i:i + 1], alone), i
        if i < 65:
            assert _same(small[i:i + 1], alone), i
    # the same row at another place of a 65-row call
    assert _same(ops.linear_fwd_bm(x[235:300], *packed, bias, tiled=True)[64:65], big[299:300])
    # leading dims
    assert _same(ops.linear_fwd_bm(x[:12].reshape(3, 4, -1), *packed, bias, tiled=True).reshape(12, -1), big[:12])


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_rows_and_an_offset_start(dtype):
    """ldx > K, ldy > N and X starting 16 bytes into its allocation, through the C entry point, at M = 65"""
    from vlmc import _lib, ops
    n, k, m = 33, 40, 65
    (values, meta, offs, rowptr), dense, _keep, bias, x = _case(n, k, dtype)
    ldx, ldy = k + 16, n + 3
    xbuf = torch.zeros(8 + m * ldx, dtype=dtype, device=DEV)
    xs = xbuf[8:].view(m, ldx)
    xs[:, :k] = x[:m]
    xs[:, k:] = float("nan")                                                  # never read
    assert xs.data_ptr() % 16 == 0 and xs.data_ptr() == xbuf.data_ptr() + 16
    y = torch.full((m, ldy), 7.0, dtype=dtype, device=DEV)
    _lib.check(_lib.load().vlmc_linear_fwd_bm_tiled(xs.data_ptr(), values.data_ptr(), meta.data_ptr(), offs.data_ptr(), rowptr.data_ptr(),
                                                    values.numel() - 16, bias.data_ptr(), ops._DT[dtype], m, n, k, ldx, y.data_ptr(), ldy,
                                                    ops._stream()))
    want = ops.linear_fwd(x[:m], dense, bias)
    assert not bool(torch.isnan(want).any())
    assert _same(y[:, :n], want)
    assert bool((y[:, n:] == 7.0).all())                                      # nothing written past a row's N outputs
    # the same rows as a strided view, through the wrapper
    assert _same(ops.linear_fwd_bm(xs[:, :k], values, meta, offs, rowptr, bias, tiled=True), want)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_values_travel_as_they_are(dtype):
    from vlmc import ops
    n, k, m = 17, 64, 65
    gen = torch.Generator(device=DEV).manual_seed(5)
    W = (torch.randn(n, k, generator=gen, device=DEV) * 0.05).to(dtype)
    keep = torch.rand(n, k, generator=gen, device=DEV) < 0.5
    # a kept +0, a kept -0 and a kept inf: positions come from the mask, the values travel as they are
    c0, c1, c2 = (int(c) for c in keep[3].nonzero().flatten()[:3])
    W[3, c0], W[3, c1], W[3, c2] = 0.0, -0.0, float("inf")
    # an inf and a NaN of the original weight at columns the mask prunes: they are not part of the packed weight
    p0, p1 = (int(c) for c in (~keep[5]).nonzero().flatten()[:2])
    W[5, p0], W[5, p1] = float("inf"), float("nan")
    packed, dense = _pack(W, keep)
    assert int(_bits(dense)[3, c0]) == 0 and int(_bits(dense)[3, c1]) == -32768 and bool(torch.isinf(dense[3, c2]))
    assert bool(torch.isfinite(dense[5]).all())
    x = torch.randn(m, k, generator=gen, device=DEV).to(dtype)
    got, want = ops.linear_fwd_bm(x, *packed, tiled=True), ops.linear_fwd(x, dense)
    assert _same(got, want)
    assert bool(torch.isinf(want[:, 3]).all()) and bool(torch.isfinite(got[:, 5]).all())
    # rows of X that meet the kept -0 alone (+1 and -1 at its column, +0 elsewhere): the dense kernel's signs of zero
    xz = torch.zeros(m, k, dtype=dtype, device=DEV)
    xz[0, c1], xz[1, c1] = 1.0, -1.0
    assert _same(ops.linear_fwd_bm(xz, *packed, tiled=True), ops.linear_fwd(xz, dense))


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_corrupted_metadata_stays_inside_values(dtype):
    """offs and rowptr that point far past the end: the index is clamped, so nothing outside values[0, nnz + 16) is read (only reads
    are at stake: the output is the call's own)"""
    from vlmc import ops
    n, k, m = 33, 1408, 129
    (values, meta, offs, rowptr), _dense, _keep, bias, x = _case(n, k, dtype)
    nv = values.numel()
    high = offs.clone()
    high.view(torch.int16)[:] = -1                                             # 65535 kept columns before every step
    far = rowptr.clone()
    far[1::2] += 10 ** 12                                                      # beyond nnz
    far[2::4] = -10 ** 12                                                      # and below 0
    outs = []
    for fill in (float("nan"), 3.0):
        guard = torch.full((nv + 8192,), fill, dtype=dtype, device=DEV)        # values sits in the middle of the fill
        guard[4096:4096 + nv] = values
        inside = guard[4096:4096 + nv]
        assert inside.data_ptr() % 4 == 0
        per = [ops.linear_fwd_bm(x[:m], inside, meta, o, r, bias, tiled=True) for o, r in ((high, rowptr), (offs, far), (high, far))]
        torch.cuda.synchronize()
        outs.append(per)
    for a, b in zip(*outs):
        assert bool(torch.isfinite(a).all())
        assert _same(a, b)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def no_scratch_child():
    """(child process: the shared scratch weight of the unpack route does not exist yet) what a tiled forward and then an unpack-route
    forward allocate at 257 rows of a 1408 x 6144 weight"""
    from vlmc import ops
    n, k, m = 1408, 6144, 257
    gen = torch.Generator(device=DEV).manual_seed(9)
    W = (torch.randn(n, k, generator=gen, device=DEV) * 0.02).half()
    keep = torch.rand(n, k, generator=gen, device=DEV) < 0.5
    packed, dense = _pack(W, keep)
    x = torch.randn(m, k, generator=gen, device=DEV).half()
    want = ops.linear_fwd(x, dense)
    del dense, keep, W
    grown = {}
    for route in ("tiled", "unpack"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        y = ops.linear_fwd_bm(x, *packed, tiled=True) if route == "tiled" else ops.linear_fwd_bm(x, *packed, unpack=True)
        torch.cuda.synchronize()
        grown[route] = torch.cuda.max_memory_allocated() - before
        grown[route + "_same"] = _same(y, want)
        del y
    return grown


def test_no_scratch_weight(tmp_path):
    r = variant_runs.run_variants(tmp_path, "test_linearbm_tiled_gpu", "no_scratch_child", {"default": {}})["default"]
    dense_bytes, out_bytes = 1408 * 6144 * 2, 257 * 1408 * 2
    assert r["tiled"] <= out_bytes + (1 << 20) < dense_bytes, r
    assert r["unpack"] >= dense_bytes, r
    assert r["tiled_same"] and r["unpack_same"]


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_model_width_at_257_rows_through_a_packed_module(monkeypatch):
    import torch.nn as nn
    from vlmc import ops
    from vlmc.packedbm import LinearBM, pack_model_bm_
    n, k, m = 11008, 4096, 257
    gen = torch.Generator(device=DEV).manual_seed(n)
    lin = nn.Linear(k, n, bias=True, device=DEV, dtype=torch.float16)
    with torch.no_grad():
        lin.weight.copy_((torch.randn(n, k, generator=gen, device=DEV) * 0.02).half())
        lin.bias.copy_(torch.randn(n, generator=gen, device=DEV).half())
    sq = torch.rand(k, generator=gen, device=DEV) + 0.5
    keep, _ = ops.wanda_select(lin.weight.detach(), sq, "row", k=k // 2, apply_zero=False)      # Wanda's 50 % per output row
    assert int(keep.sum()) == n * k // 2
    lin.mask = keep
    x = torch.randn(m, k, generator=gen, device=DEV).half()
    want = ops.linear_fwd(x, _masked(lin.weight.detach(), keep), lin.bias.detach())
    holder = nn.ModuleDict({"fc": lin})
    assert pack_model_bm_(holder) == ["fc"] and isinstance(holder["fc"], LinearBM)
    plain, calls = ops.linear_fwd_bm, []

    def forced(x, values, meta, offs, rowptr, bias=None):
        calls.append(x.numel() // x.shape[-1])
        return plain(x, values, meta, offs, rowptr, bias, tiled=True)

    monkeypatch.setattr(ops, "linear_fwd_bm", forced)
    with torch.no_grad():
        got = holder["fc"](x)
    assert calls == [m]
    assert _same(got, want)
