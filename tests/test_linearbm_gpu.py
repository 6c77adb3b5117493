"""GPU: the packed bitmap ("bm") format end to end.  The pack / unpack kernels (vlmc_pack_bm_rows / vlmc_pack_bm / vlmc_unpack_bm) equal the
numpy restatement (tests/packbm_restatement.py) and round-trip under unstructured masks; a linear computed FROM its packed weight
(vlmc_linear_fwd_bm, `ops.linear_fwd_bm`, `packedbm.LinearBM`) gives, bit for bit, what the dense batch-invariant kernel gives on the
unpacked weight -- `ops.linear_fwd(x, ops.unpack_bm(..)[0], bias)`; a model pruned at unstructured 50 % runs, saves and reloads packed.
No tolerance anywhere: every comparison is on integer views."""
import copy
import functools

import numpy as np
import pytest
import torch

import packbm_restatement as packbm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _u16(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _masked(W, keep):
    """W . mask with +0 at the pruned positions (a product would leave -0 under a negative weight)"""
    return torch.where(keep, W, torch.zeros_like(W))


def _max_rows():
    from vlmc import ops
    return ops.linear_fwd_bm_max_rows()


def _mask(W, gen, mode="row", density=0.5):
    """a keep mask of `W` from the selection kernel at kept density `density` ("row": the same count in every row; "matrix": ragged rows);
    W is left as it was"""
    from vlmc import ops
    n, k = W.shape
    sq = torch.rand(k, generator=gen, device=DEV) + 0.5
    pruned = k - int(round(k * density)) if mode == "row" else n * k - int(round(n * k * density))
    keep, _ = ops.wanda_select(W, sq, mode, k=pruned, apply_zero=False)
    return keep


def _pruned(n, k, dtype, gen, scale=0.05, mode="row", density=0.5):
    """(packed = (values, meta, offs, rowptr), dense W . mask, mask) of a random weight pruned unstructured"""
    from vlmc import ops
    W = (torch.randn(n, k, generator=gen, device=DEV) * scale).to(dtype)
    keep = _mask(W, gen, mode, density)
    packed = ops.pack_bm(W, keep)
    dense, k2 = ops.unpack_bm(*packed)
    assert torch.equal(k2, keep) and _same(dense, _masked(W, keep))
    return packed, dense, keep


@functools.lru_cache(maxsize=None)
def _case(n, k, dtype):
    """one pruned weight, bias and 300 rows of activations per (N, K, dtype), shared by the tests below and never written to"""
    gen = torch.Generator(device=DEV).manual_seed(1000 * n + k)
    packed, dense, keep = _pruned(n, k, dtype, gen)
    bias = torch.randn(n, generator=gen, device=DEV).to(dtype)
    x = torch.randn(300, k, generator=gen, device=DEV).to(dtype)
    return packed, dense, keep, bias, x


# ---- pack and unpack -------------------------------------------------------------------------------------------------------
def test_kernels_equal_the_restatement_and_round_trip():
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(0)
    codes = set()
    for dtype in DTYPES:
        for out_f, in_f in ((5, 8), (33, 40), (128, 1408), (64, 2048)):
            for mode in ("row", "matrix"):
                W = torch.randn(out_f, in_f, generator=g, device=DEV).to(dtype)
                W[0, :8] = 0                                                   # kept zeros stay kept: positions come from the mask
                keep = _mask(W, g, mode)
                keep[1] = False                                                # one row empty
                keep[out_f - 1] = True                                         # and one full
                values, meta, offs, rowptr = ops.pack_bm(W, keep)
                ov, om, oo, orp = packbm.pack(_u16(W), keep.cpu().numpy())
                assert np.array_equal(_u16(values), ov) and np.array_equal(meta.cpu().numpy(), om), (out_f, in_f, mode)
                assert np.array_equal(_u16(offs), oo) and np.array_equal(rowptr.cpu().numpy(), orp), (out_f, in_f, mode)
                nnz = int(keep.sum())
                assert int(rowptr[-1]) == nnz == values.numel() - 16
                nbytes = sum(t.numel() * t.element_size() for t in (values, meta, offs, rowptr))
                assert nbytes == (nnz + 16) * 2 + out_f * in_f // 8 + 2 * out_f * ((in_f + 31) // 32) + 8 * (out_f + 1)
                w2, k2 = ops.unpack_bm(values, meta, offs, rowptr)
                ow, ok, obad = packbm.unpack(ov, om, oo, orp)
                assert obad == 0 and np.array_equal(_u16(w2), ow) and np.array_equal(k2.cpu().numpy(), ok)
                assert torch.equal(k2, keep) and _same(w2, _masked(W, keep))
                assert ops.unpack_bm(values, meta, offs, rowptr, want_mask=False)[1] is None
                codes |= set(meta.unique().tolist())
    assert len(codes) == 256                                                   # every metadata byte went through both kernels
    with pytest.raises(TypeError):
        ops.pack_bm(W.float(), keep)
    with pytest.raises(TypeError):
        ops.pack_bm(W[:, :12], keep[:, :12])


@pytest.mark.parametrize("dtype", DTYPES)
def test_unpack_with_corrupted_metadata_raises_and_stays_inside_values(dtype):
    from vlmc import ops
    gen = torch.Generator(device=DEV).manual_seed(4)
    W = (torch.randn(33, 1408, generator=gen, device=DEV) * 0.05).to(dtype)
    keep = _mask(W, gen)
    values, meta, offs, rowptr = ops.pack_bm(W, keep)
    n = values.numel()
    guard = torch.full((n + 8192,), float("nan"), dtype=dtype, device=DEV)     # values sits in the middle of NaNs
    guard[4096:4096 + n] = values
    inside = guard[4096:4096 + n]
    assert inside.data_ptr() % 4 == 0
    from vlmc import _lib

    def raw_unpack(o, r):
        """through the C entry point: the output and the bad count, whatever the metadata holds"""
        w = torch.empty(33, 1408, dtype=dtype, device=DEV)
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        _lib.check(_lib.load().vlmc_unpack_bm(inside.data_ptr(), meta.data_ptr(), o.data_ptr(), r.data_ptr(), n - 16, ops._DT[dtype], 33, 1408,
                                              w.data_ptr(), 1408, None, 0, bad.data_ptr(), ops._stream()))
        return w, int(bad.item())

    w, bad = raw_unpack(offs, rowptr)
    assert bad == 0 and _same(w, _masked(W, keep))
    high = offs.clone()
    high.view(torch.int16)[:, 1:] = -1                                         # 65535 kept columns before every later step: far past the end
    w, bad = raw_unpack(high, rowptr)
    assert bad == 33 * (1408 // 32 - 1) and not bool(torch.isnan(w).any())
    far = rowptr.clone()
    far[5] += 10 ** 9
    far[9] = -10 ** 9
    w, bad = raw_unpack(offs, far)
    assert bad == 4 and not bool(torch.isnan(w).any())                         # rows 4, 5, 8 and 9 have a wrong rowptr pair
    for o, r in ((high, rowptr), (offs, far)):
        with pytest.raises(ValueError, match="never writes"):
            ops.unpack_bm(inside, meta, o, r)
    short = rowptr.clone()
    short[-1] -= 1
    with pytest.raises(ValueError, match="never writes"):
        ops.unpack_bm(inside, meta, offs, short)                               # rowptr[N] != nnz


# ---- the forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [8, 40, 64, 1408])
@pytest.mark.parametrize("n", [1, 5, 16, 17, 33])
def test_small_shapes_bit_for_bit(n, k, dtype):
    from vlmc import ops
    packed, dense, _keep, bias, x = _case(n, k, dtype)
    mr = _max_rows()
    for m in sorted({1, 2, 15, 16, 17, mr - 1, mr, mr + 1, 300}):
        for b in (None, bias):
            want = ops.linear_fwd(x[:m], dense, b)
            got = ops.linear_fwd_bm(x[:m], *packed, b)
            assert _same(got, want), (n, k, m, b is not None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["row", "matrix"])
@pytest.mark.parametrize("density", [0.5, 0.1, 0.9])
def test_densities_bit_for_bit(density, mode, dtype):
    from vlmc import ops
    gen = torch.Generator(device=DEV).manual_seed(int(density * 100))
    packed, dense, _keep = _pruned(33, 1408, dtype, gen, mode=mode, density=density)
    bias = torch.randn(33, generator=gen, device=DEV).to(dtype)
    x = torch.randn(_max_rows(), 1408, generator=gen, device=DEV).to(dtype)
    for m in sorted({1, 16, 17, _max_rows()}):
        assert _same(ops.linear_fwd_bm(x[:m], *packed, bias), ops.linear_fwd(x[:m], dense, bias)), m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["odd_rowptr", "empty_first_and_last"])
def test_fixed_layouts(layout, dtype):
    from vlmc import ops
    n, k = 17, 64
    gen = torch.Generator(device=DEV).manual_seed(6)
    W = (torch.randn(n, k, generator=gen, device=DEV) * 0.05).to(dtype)
    keep = torch.rand(n, k, generator=gen, device=DEV) < 0.5
    if layout == "odd_rowptr":
        # row 0 keeps one column, every later row an even number: every row after the first starts at an odd index
        keep[0] = False
        keep[0, 3] = True
        for r in range(1, n):
            if int(keep[r].sum()) % 2:
                keep[r, 0] = ~keep[r, 0]
    else:
        keep[0] = False
        keep[n - 1] = False
    packed = ops.pack_bm(W, keep)
    rowptr = packed[3].cpu()
    if layout == "odd_rowptr":
        assert bool((rowptr[1:] % 2 == 1).all())
    else:
        assert int(rowptr[0]) == int(rowptr[1]) == 0 and int(rowptr[n - 1]) == int(rowptr[n])
    dense, k2 = ops.unpack_bm(*packed)
    assert torch.equal(k2, keep) and _same(dense, _masked(W, keep))
    x = torch.randn(20, k, generator=gen, device=DEV).to(dtype)
    for m in (1, 16, 20):
        assert _same(ops.linear_fwd_bm(x[:m], *packed), ops.linear_fwd(x[:m], dense)), m


@pytest.mark.parametrize("n,k", [(11008, 4096), (4096, 11008)])
def test_model_widths_at_16_rows(n, k):
    from vlmc import ops
    gen = torch.Generator(device=DEV).manual_seed(n)
    packed, dense, _keep = _pruned(n, k, torch.float16, gen, scale=0.02)
    x = torch.randn(16, k, generator=gen, device=DEV).half()
    assert _same(ops.linear_fwd_bm(x, *packed), ops.linear_fwd(x, dense))


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_rows_and_an_offset_start(dtype):
    """ldx > K, ldy > N and X starting 16 bytes into its allocation, through the C entry point"""
    from vlmc import _lib, ops
    n, k, m = 33, 40, 15
    (values, meta, offs, rowptr), dense, _keep, bias, x = _case(n, k, dtype)
    ldx, ldy = k + 16, n + 3
    xbuf = torch.zeros(8 + m * ldx, dtype=dtype, device=DEV)
    xs = xbuf[8:].view(m, ldx)
    xs[:, :k] = x[:m]
    xs[:, k:] = float("nan")                                                  # never read
    assert xs.data_ptr() % 16 == 0 and xs.data_ptr() == xbuf.data_ptr() + 16
    y = torch.full((m, ldy), 7.0, dtype=dtype, device=DEV)
    _lib.check(_lib.load().vlmc_linear_fwd_bm(xs.data_ptr(), values.data_ptr(), meta.data_ptr(), offs.data_ptr(), rowptr.data_ptr(),
                                              values.numel() - 16, bias.data_ptr(), ops._DT[dtype], m, n, k, ldx, y.data_ptr(), ldy, None, 0,
                                              ops._stream()))
    assert _same(y[:, :n], ops.linear_fwd(x[:m], dense, bias))
    assert bool((y[:, n:] == 7.0).all())                                      # nothing written past a row's N outputs
    # the same rows as a strided view, through the wrapper
    assert _same(ops.linear_fwd_bm(xs[:, :k], values, meta, offs, rowptr, bias), ops.linear_fwd(x[:m], dense, bias))


@pytest.mark.parametrize("dtype", DTYPES)
def test_kept_zeros_and_an_inf_at_a_pruned_column(dtype):
    from vlmc import ops
    n, k = 17, 64
    gen = torch.Generator(device=DEV).manual_seed(5)
    W = (torch.randn(n, k, generator=gen, device=DEV) * 0.05).to(dtype)
    keep = _mask(W, gen)
    # a kept +0 and a kept -0: positions come from the mask, the values travel as they are
    c0, c1 = (int(c) for c in keep[3].nonzero().flatten()[:2])
    W[3, c0], W[3, c1] = 0.0, -0.0
    packed = ops.pack_bm(W, keep)
    dense, k2 = ops.unpack_bm(*packed)
    assert torch.equal(k2, keep) and int(_bits(dense)[3, c0]) == 0 and int(_bits(dense)[3, c1]) == -32768
    x = torch.randn(20, k, generator=gen, device=DEV).to(dtype)
    for m in (1, 16, 20):
        assert _same(ops.linear_fwd_bm(x[:m], *packed), ops.linear_fwd(x[:m], dense))
    # inf in X at a column that row 5's mask prunes (and other rows keep): the dense layer multiplies inf by the stored zero
    col = int((~keep[5]).nonzero().flatten()[0])
    xi = x[:16].clone()
    xi[2, col] = float("inf")
    got, want = ops.linear_fwd_bm(xi, *packed), ops.linear_fwd(xi, dense)
    assert bool(torch.isnan(want[2, 5])) and not bool(torch.isnan(want[3]).any())
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert torch.equal(_bits(got)[ok], _bits(want)[ok])


@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_kernel_and_unpack_route_agree(dtype):
    from vlmc import ops
    packed, dense, _keep, bias, x = _case(33, 1408, dtype)
    for m in (1, 16, _max_rows()):
        a = ops.linear_fwd_bm(x[:m], *packed, bias)
        b = ops.linear_fwd_bm(x[:m], *packed, bias, unpack=True)
        assert _same(a, b) and _same(a, ops.linear_fwd(x[:m], dense, bias))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_do_not_depend_on_the_batch(dtype):
    from vlmc import ops
    packed, _dense, _keep, bias, x = _case(33, 1408, dtype)
    mr = _max_rows()
    big, small = ops.linear_fwd_bm(x, *packed, bias), ops.linear_fwd_bm(x[:mr], *packed, bias)
    for i in (0, 7, mr - 1):
        alone = ops.linear_fwd_bm(x[i:i + 1], *packed, bias)
        assert _same(big[i:i + 1], alone) and _same(small[i:i + 1], alone)
    for i in (mr, 299):
        assert _same(big[i:i + 1], ops.linear_fwd_bm(x[i:i + 1], *packed, bias))
    # leading dims
    assert _same(ops.linear_fwd_bm(x[:12].reshape(3, 4, -1), *packed, bias).reshape(12, -1), big[:12])


def test_forward_allocates_less_than_the_dense_weight():
    from vlmc import ops
    from vlmc.packedbm import LinearBM
    n = k = 4096
    gen = torch.Generator(device=DEV).manual_seed(9)
    packed, dense, _keep = _pruned(n, k, torch.float16, gen, scale=0.02)
    lin = LinearBM(*packed)
    x = torch.randn(16, k, generator=gen, device=DEV).half()
    want = ops.linear_fwd(x, dense)
    del dense, _keep
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    y = lin(x)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert grown < n * k * 2, grown
    assert _same(y, want)


# ---- modules ---------------------------------------------------------------------------------------------------------------
def _toy_unstructured():
    """the 16-bit toy InstructBLIP (fp16 ViT, bf16 T5) pruned at unstructured 50 % by the drop-in Wanda pruner, and one batch"""
    from lavis.compression import load_pruner
    import toy_models
    model = toy_models.init_toy(toy_models.ToyBlipT5(vit_dtype=torch.float16, t5_dtype=torch.bfloat16), seed=7).eval().to(DEV)
    batches = [{k: t.to(DEV) for k, t in b.items()} for b in toy_models.make_batches(4, seed=11)]
    spec = "2-0.5-1.0-1.0"
    cfg = dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method="wanda", vit_pruning_method="wanda", num_samples=4,
               max_sparsity_per_layer=1.01)
    pruned, _ = load_pruner("blipt5_wanda_pruner", model, batches, cfg=cfg).prune()
    return pruned, batches[0]


def _invariant_forward(model, batch):
    """one forward with every plain linear on ops.linear_fwd"""
    from vlmc import forward
    import torch.nn as nn
    linears = [m for m in model.modules() if type(m) is nn.Linear]
    with torch.no_grad(), forward.invariant_linears(linears):
        return model(batch)["logits"]


def _masks(model):
    return {n: m.mask for n, m in model.named_modules() if torch.is_tensor(getattr(m, "mask", None))}


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16) if a.element_size() == 2 else a,
                                                                     b.view(torch.int16) if b.element_size() == 2 else b)


def test_packed_model_forward_unpack_and_loaders():
    from vlmc import formats
    from vlmc.packed24 import is_mask_24
    from vlmc.packed48 import is_mask_48
    from vlmc.packedbm import LinearBM, is_mask_bm, pack_model_bm_, unpack_model_bm_
    pruned, batch = _toy_unstructured()
    masks = _masks(pruned)
    assert len(masks) == 2 * 4 + 2 * 7 + 2 * 11
    assert all(is_mask_bm(m, m.shape) for m in masks.values())
    assert not any(is_mask_24(m, m.shape) or is_mask_48(m, m.shape) for m in masks.values())      # what the n:m packers cannot take
    dense_state = {k: v.clone() for k, v in pruned.state_dict().items()}
    fresh = copy.deepcopy(pruned)                                              # for the loaders below (masks travel as attributes)
    want = _invariant_forward(pruned, batch)
    assert want.dtype == torch.float32 and bool(torch.isfinite(want).all())
    state = dict(dense_state)
    state.update({n + ".mask": m for n, m in masks.items()})

    # ---- pack in place: the same forward from fewer bytes
    names = pack_model_bm_(pruned)
    assert sorted(names) == sorted(masks)
    assert all(isinstance(pruned.get_submodule(n), LinearBM) for n in names)
    assert sum(isinstance(m, LinearBM) for m in pruned.modules()) == len(masks)
    got = _invariant_forward(pruned, batch)                                    # (t5_proj stays a plain linear)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    packed_live = {k: v.clone() for k, v in pruned.state_dict().items()}
    for n in names:
        lin = pruned.get_submodule(n)
        assert sum(t.numel() * t.element_size() for t in lin._packed()) < 2 * lin.in_features * lin.out_features

    # ---- and back: weights and masks bit for bit
    assert sorted(unpack_model_bm_(pruned)) == sorted(names)
    back = pruned.state_dict()
    assert list(back) == list(dense_state)
    for k, v in dense_state.items():
        assert _eq(back[k], v), k
    for n, m in masks.items():
        assert torch.equal(pruned.get_submodule(n).mask, m), n

    # ---- pack_state_dict_bm -> load_packed_bm into a dense copy
    packed = formats.pack_state_dict_bm(state)
    assert sum(k.endswith(formats.PACKED_VALUES_BM) for k in packed) == len(masks) and not any(k.endswith(".mask") for k in packed)
    assert sum(k.endswith(formats.PACKED_ROWPTR_BM) for k in packed) == sum(k.endswith(formats.PACKED_OFFS_BM) for k in packed) == len(masks)
    loaded = copy.deepcopy(fresh)
    formats.load_packed_bm(loaded, packed)
    assert sum(isinstance(m, LinearBM) for m in loaded.modules()) == len(masks)
    assert torch.equal(_invariant_forward(loaded, batch).view(torch.int32), want.view(torch.int32))
    live = loaded.state_dict()
    assert live.keys() == packed.keys() == packed_live.keys()
    for k in packed:
        assert _eq(live[k], packed[k]) and _eq(live[k], packed_live[k]), k
    again = formats.pack_state_dict_bm(formats.unpack_state_dict_bm(live))
    assert again.keys() == live.keys() and all(_eq(again[k], live[k]) for k in live)
    bad = dict(packed)
    key = next(k for k in bad if k.endswith(formats.PACKED_OFFS_BM))
    bad[key] = bad[key].clone()
    bad[key].view(torch.int16)[0, -1] += 1                                     # one wrong offs entry
    with pytest.raises(ValueError, match="weight_offsbm / .*weight_rowptrbm hold entries that pack_bm never writes"):
        formats.load_packed_bm(copy.deepcopy(fresh), bad)

    # ---- the reference's reload keeps the zeros and drops the masks: from_zeros
    reloaded = copy.deepcopy(fresh)
    for m in reloaded.modules():
        if torch.is_tensor(getattr(m, "mask", None)):
            del m.mask
    assert pack_model_bm_(reloaded) == []
    got_names = pack_model_bm_(reloaded, from_zeros=True)
    assert set(masks) <= set(got_names)
    assert torch.equal(_invariant_forward(reloaded, batch).view(torch.int32), want.view(torch.int32))


def test_fp32_and_dense_masks_are_left_alone_and_the_n_m_packers_go_first():
    import torch.nn as nn
    from vlmc.packed24 import Linear24, pack_model_24_
    from vlmc.packedbm import LinearBM, pack_model_bm_
    g = torch.Generator(device=DEV).manual_seed(8)
    model = nn.ModuleDict({k: nn.Linear(64, 32) for k in "abcde"}).to(DEV)
    for k in "bcde":
        model[k].to(torch.bfloat16)
    model["a"].mask = torch.rand(32, 64, device=DEV, generator=g) > 0.5                             # fp32: not packed
    model["b"].mask = torch.rand(32, 64, device=DEV, generator=g) > 0.02                            # 98 % kept: above break-even
    model["c"].mask = torch.rand(32, 64, device=DEV, generator=g) > 0.5                             # unstructured
    model["d"].mask = torch.tensor([True, False, False, True], device=DEV).repeat(32, 16)           # 2:4
    assert pack_model_24_(model) == ["d"]
    x = torch.randn(5, 64, device=DEV, generator=g).to(torch.bfloat16)
    from vlmc import ops
    want = {k: ops.linear_fwd(x, _masked(model[k].weight.detach(), model[k].mask), model[k].bias.detach()) for k in "c"}
    assert pack_model_bm_(model) == ["c"]                                                           # e has no mask
    assert type(model["a"]) is nn.Linear and type(model["b"]) is nn.Linear and type(model["e"]) is nn.Linear
    assert isinstance(model["c"], LinearBM) and isinstance(model["d"], Linear24)
    assert _same(model["c"](x), want["c"])
    # without the 2:4 walk first, the 2:4 linear is a mask like any other
    other = nn.ModuleDict(dict(d=nn.Linear(64, 32).to(torch.bfloat16))).to(DEV)
    other["d"].mask = torch.tensor([True, False, False, True], device=DEV).repeat(32, 16)
    assert pack_model_bm_(other) == ["d"] and isinstance(other["d"], LinearBM)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_merged_sparse_lora_linear_converts(dtype):
    from lavis.peft.src.peft.tuners.lora import Linear as LoraLinear
    from vlmc import ops
    from vlmc.packedbm import LinearBM, pack_model_bm_
    gen = torch.Generator(device=DEV).manual_seed(3)
    holder = torch.nn.Module()
    holder.lin = LoraLinear(64, 48, r=4, lora_alpha=8, bias=True, merge_weights=False).to(DEV)
    lin = holder.lin
    lin.sparse = True
    with torch.no_grad():
        lin.weight.copy_(torch.randn(48, 64, generator=gen, device=DEV) * 0.05)
        lin.lora_B.weight.copy_(torch.randn(48, 4, generator=gen, device=DEV) * 0.05)
    lin.weight.data, lin.bias.data = lin.weight.data.to(dtype), lin.bias.data.to(dtype)      # (the LoRA factors stay fp32 parameters)
    keep = _mask(lin.weight.data, gen)
    lin.mask = keep
    assert pack_model_bm_(holder) == []                                        # a live adapter: not packable
    lin.merge()
    W, bias = lin.weight.data.clone(), lin.bias.data.clone()
    assert pack_model_bm_(holder) == ["lin"] and isinstance(holder.lin, LinearBM)
    x = torch.randn(9, 64, generator=gen, device=DEV).to(dtype)
    with torch.no_grad():
        assert _same(holder.lin(x, False), ops.linear_fwd(x, _masked(W, keep), bias))
