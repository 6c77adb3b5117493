"""GPU: the packed 4:8 format end to end.  The pack / unpack kernels (vlmc_pack_48 / vlmc_unpack_48) equal the numpy restatement
(tests/pack48_restatement.py) and round-trip; a linear computed FROM its packed 4:8 weight (vlmc_linear_fwd_48, `ops.linear_fwd_48`,
`packed48.Linear48`) gives, bit for bit, what the dense batch-invariant kernel gives on the unpacked weight --
`ops.linear_fwd(x, ops.unpack_48(values, meta)[0], bias)`; a 4:8-pruned model runs, saves and reloads packed.  No tolerance
anywhere: every comparison is on integer views."""
import copy
import functools

import numpy as np
import pytest
import torch

import pack48_restatement as pack48

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _u16(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _max_rows():
    from vlmc import ops
    return ops.linear_fwd_24_max_rows()


def _pruned(n, k, dtype, gen, scale=0.05):
    """(values, meta, dense W . mask, mask) of a random weight pruned 4:8 by the n:m rule"""
    from vlmc import ops
    W = (torch.randn(n, k, generator=gen, device=DEV) * scale).to(dtype)
    sq = torch.rand(k, generator=gen, device=DEV) + 0.5
    keep, _ = ops.wanda_select(W, sq, "nm", n=4, m=8)
    assert bool((keep.reshape(n, -1, 8).sum(-1) == 4).all())
    values, meta = ops.pack_48(W, keep)
    dense, k2 = ops.unpack_48(values, meta)
    assert torch.equal(k2, keep) and _same(dense, W)
    return values, meta, dense, keep


@functools.lru_cache(maxsize=None)
def _case(n, k, dtype):
    """one pruned weight, bias and 300 rows of activations per (N, K, dtype), shared by the tests below and never written to"""
    gen = torch.Generator(device=DEV).manual_seed(1000 * n + k)
    values, meta, dense, keep = _pruned(n, k, dtype, gen)
    bias = torch.randn(n, generator=gen, device=DEV).to(dtype)
    x = torch.randn(300, k, generator=gen, device=DEV).to(dtype)
    return values, meta, dense, keep, bias, x


# ---- pack and unpack -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernels_equal_the_restatement_and_round_trip(dtype):
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(0)
    codes = set()
    for out_f, in_f in ((5, 8), (33, 64), (128, 1408), (64, 2048)):
        W = torch.randn(out_f, in_f, generator=g, device=DEV).to(dtype)
        W[0, :8] = 0                                                       # kept zeros stay kept: positions come from the mask
        sq = torch.rand(in_f, generator=g, device=DEV) + 0.5
        Wp = W.clone()
        keep, _ = ops.wanda_select(Wp, sq, "nm", n=4, m=8)
        values, meta = ops.pack_48(Wp, keep)
        ov, om, bad = pack48.pack(_u16(Wp), keep.cpu().numpy())
        assert bad == 0
        assert np.array_equal(_u16(values), ov) and np.array_equal(meta.cpu().numpy(), om)
        w2, k2 = ops.unpack_48(values, meta)
        ow, ok, obad = pack48.unpack(ov, om)
        assert obad == 0 and np.array_equal(_u16(w2), ow) and np.array_equal(k2.cpu().numpy(), ok)
        assert torch.equal(k2, keep) and torch.equal(w2.view(torch.int16), Wp.view(torch.int16))
        assert ops.unpack_48(values, meta, want_mask=False)[1] is None
        assert values.numel() * 2 + meta.numel() == W.numel() * 2 * 9 // 16
        codes |= set(meta.unique().tolist())
    assert len(codes) == 70 and all(bin(c).count("1") == 4 for c in codes)   # every valid metadata byte went through both kernels
    with pytest.raises(ValueError, match="not a 4:8 mask"):
        ops.pack_48(W, torch.ones_like(W, dtype=torch.bool))
    with pytest.raises(TypeError):
        ops.pack_48(W.float(), keep)
    with pytest.raises(ValueError, match="never writes"):
        ops.unpack_48(values, torch.zeros_like(meta))                      # popcount 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_2_4_mask_packs_as_4_8(dtype):
    from vlmc import ops
    g = torch.Generator(device=DEV).manual_seed(2)
    W = torch.randn(17, 64, generator=g, device=DEV).to(dtype)
    keep, _ = ops.wanda_select(W, torch.ones(64, device=DEV), "nm", n=2, m=4)
    values, meta = ops.pack_48(W, keep)
    v24, _m24 = ops.pack_24(W, keep)
    assert _same(values, v24)                                              # the same kept values in the same order; only the metadata differs
    w2, k2 = ops.unpack_48(values, meta)
    assert torch.equal(k2, keep) and _same(w2, W)
    x = torch.randn(5, 64, generator=g, device=DEV).to(dtype)
    assert _same(ops.linear_fwd_48(x, values, meta), ops.linear_fwd(x, w2))


# ---- the forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [8, 40, 64, 1408])
@pytest.mark.parametrize("n", [1, 5, 16, 17, 33])
def test_small_shapes_bit_for_bit(n, k, dtype):
    from vlmc import ops
    values, meta, dense, _keep, bias, x = _case(n, k, dtype)
    mr = _max_rows()
    for m in sorted({1, 2, 15, 16, 17, mr - 1, mr, mr + 1, 300}):
        for b in (None, bias):
            want = ops.linear_fwd(x[:m], dense, b)
            got = ops.linear_fwd_48(x[:m], values, meta, b)
            assert _same(got, want), (n, k, m, b is not None)


@pytest.mark.parametrize("n,k", [(11008, 4096), (4096, 11008)])
def test_model_widths_at_16_rows(n, k):
    from vlmc import ops
    gen = torch.Generator(device=DEV).manual_seed(n)
    values, meta, dense, _keep = _pruned(n, k, torch.float16, gen, scale=0.02)
    x = torch.randn(16, k, generator=gen, device=DEV).half()
    assert _same(ops.linear_fwd_48(x, values, meta), ops.linear_fwd(x, dense))


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_rows_and_an_offset_start(dtype):
    """ldx > K, ldy > N and X starting 16 bytes into its allocation, through the C entry point"""
    from vlmc import _lib, ops
    n, k, m = 33, 40, 17
    values, meta, dense, _keep, bias, x = _case(n, k, dtype)
    ldx, ldy = k + 16, n + 3
    xbuf = torch.zeros(8 + m * ldx, dtype=dtype, device=DEV)
    xs = xbuf[8:].view(m, ldx)
    xs[:, :k] = x[:m]
    xs[:, k:] = float("nan")                                                  # never read
    assert xs.data_ptr() % 16 == 0 and xs.data_ptr() == xbuf.data_ptr() + 16
    y = torch.full((m, ldy), 7.0, dtype=dtype, device=DEV)
    _lib.check(_lib.load().vlmc_linear_fwd_48(xs.data_ptr(), values.data_ptr(), meta.data_ptr(), bias.data_ptr(), ops._DT[dtype], m, n, k, ldx,
                                              y.data_ptr(), ldy, None, 0, ops._stream()))
    assert _same(y[:, :n], ops.linear_fwd(x[:m], dense, bias))
    assert bool((y[:, n:] == 7.0).all())                                      # nothing written past a row's N outputs
    # the same rows as a strided view, through the wrapper
    assert _same(ops.linear_fwd_48(xs[:, :k], values, meta, bias), ops.linear_fwd(x[:m], dense, bias))


@pytest.mark.parametrize("dtype", DTYPES)
def test_kept_zeros_and_an_inf_at_a_pruned_column(dtype):
    from vlmc import ops
    n, k = 17, 64
    gen = torch.Generator(device=DEV).manual_seed(5)
    W = (torch.randn(n, k, generator=gen, device=DEV) * 0.05).to(dtype)
    keep, _ = ops.wanda_select(W, torch.ones(k, device=DEV), "nm", n=4, m=8)
    # a kept +0 and a kept -0: positions come from the mask, the values travel as they are
    c0, c1 = (int(c) for c in keep[3].nonzero().flatten()[:2])
    W[3, c0], W[3, c1] = 0.0, -0.0
    values, meta = ops.pack_48(W, keep)
    dense, k2 = ops.unpack_48(values, meta)
    assert torch.equal(k2, keep) and int(_bits(dense)[3, c0]) == 0 and int(_bits(dense)[3, c1]) == -32768
    x = torch.randn(20, k, generator=gen, device=DEV).to(dtype)
    for m in (1, 16, 20):
        assert _same(ops.linear_fwd_48(x[:m], values, meta), ops.linear_fwd(x[:m], dense))
    # inf in X at a column that row 5's mask prunes (and other rows keep): the dense layer multiplies inf by the stored zero
    col = int((~keep[5]).nonzero().flatten()[0])
    xi = x.clone()
    xi[2, col] = float("inf")
    got, want = ops.linear_fwd_48(xi, values, meta), ops.linear_fwd(xi, dense)
    assert bool(torch.isnan(want[2, 5])) and not bool(torch.isnan(want[3]).any())
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert torch.equal(_bits(got)[ok], _bits(want)[ok])


@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_kernel_and_unpack_route_agree(dtype):
    from vlmc import ops
    values, meta, dense, _keep, bias, x = _case(33, 1408, dtype)
    for m in (1, 16, _max_rows()):
        a = ops.linear_fwd_48(x[:m], values, meta, bias)
        b = ops.linear_fwd_48(x[:m], values, meta, bias, unpack=True)
        assert _same(a, b) and _same(a, ops.linear_fwd(x[:m], dense, bias))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_do_not_depend_on_the_batch(dtype):
    from vlmc import ops
    values, meta, _dense, _keep, bias, x = _case(33, 1408, dtype)
    mr = _max_rows()
    big, small = ops.linear_fwd_48(x, values, meta, bias), ops.linear_fwd_48(x[:mr], values, meta, bias)
    for i in (0, 7, 16, mr - 1):
        alone = ops.linear_fwd_48(x[i:i + 1], values, meta, bias)
        assert _same(big[i:i + 1], alone) and _same(small[i:i + 1], alone)
    for i in (mr, 299):
        assert _same(big[i:i + 1], ops.linear_fwd_48(x[i:i + 1], values, meta, bias))
    # leading dims
    assert _same(ops.linear_fwd_48(x[:12].reshape(3, 4, -1), values, meta, bias).reshape(12, -1), big[:12])


def test_forward_allocates_less_than_the_dense_weight():
    from vlmc import ops
    from vlmc.packed48 import Linear48
    n = k = 4096
    gen = torch.Generator(device=DEV).manual_seed(9)
    values, meta, dense, _keep = _pruned(n, k, torch.float16, gen, scale=0.02)
    lin = Linear48(values, meta)
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
def _toy_4_8():
    """the 16-bit toy InstructBLIP (fp16 ViT, bf16 T5) pruned 4:8 by the drop-in Wanda pruner, and one batch"""
    from lavis.compression import load_pruner
    import toy_models
    model = toy_models.init_toy(toy_models.ToyBlipT5(vit_dtype=torch.float16, t5_dtype=torch.bfloat16), seed=7).eval().to(DEV)
    batches = [{k: t.to(DEV) for k, t in b.items()} for b in toy_models.make_batches(4, seed=11)]
    spec = "2-0.5-1.0-1.0"
    cfg = dict(t5_prune_spec=spec, vit_prune_spec=spec, t5_pruning_method="wanda", vit_pruning_method="wanda", num_samples=4,
               prune_n=4, prune_m=8, max_sparsity_per_layer=1.01)
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


def test_packed_model_forward_unpack_and_loaders():
    from vlmc import formats
    from vlmc.packed24 import Linear24, pack_model_24_
    from vlmc.packed48 import Linear48, is_mask_48, pack_model_48_, unpack_model_48_
    pruned, batch = _toy_4_8()
    masks = _masks(pruned)
    assert len(masks) == 2 * 4 + 2 * 7 + 2 * 11
    assert all(is_mask_48(m, m.shape) for m in masks.values())
    dense_state = {k: v.clone() for k, v in pruned.state_dict().items()}
    fresh = copy.deepcopy(pruned)                                              # for the loaders below (masks travel as attributes)
    want = _invariant_forward(pruned, batch)
    assert want.dtype == torch.float32 and bool(torch.isfinite(want).all())

    # ---- 2:4 is unaffected: nothing here is a 2:4 linear, so the 2:4 walk and the 2:4 state-dict packer pass it all by
    state = dict(dense_state)
    state.update({n + ".mask": m for n, m in masks.items()})
    assert pack_model_24_(pruned) == [] and not any(isinstance(m, Linear24) for m in pruned.modules())
    left = formats.pack_state_dict_24(state)
    assert left.keys() == state.keys() and all(left[k] is state[k] for k in state)

    # ---- pack in place: the same forward from 9 / 16 of the bytes
    names = pack_model_48_(pruned)
    assert sorted(names) == sorted(masks)
    assert all(isinstance(pruned.get_submodule(n), Linear48) for n in names)
    assert sum(isinstance(m, Linear48) for m in pruned.modules()) == len(masks)
    got = _invariant_forward(pruned, batch)                                    # (t5_proj stays a plain linear)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    packed_live = {k: v.clone() for k, v in pruned.state_dict().items()}

    # ---- and back: weights and masks bit for bit
    assert sorted(unpack_model_48_(pruned)) == sorted(names)
    back = pruned.state_dict()
    assert list(back) == list(dense_state)
    for k, v in dense_state.items():
        assert torch.equal(back[k].view(torch.int16) if v.dtype in DTYPES else back[k], v.view(torch.int16) if v.dtype in DTYPES else v), k
    for n, m in masks.items():
        assert torch.equal(pruned.get_submodule(n).mask, m), n

    # ---- pack_state_dict_48 -> load_packed_48 into a dense copy
    packed = formats.pack_state_dict_48(state)
    assert sum(k.endswith(formats.PACKED_VALUES_48) for k in packed) == len(masks) and not any(k.endswith(".mask") for k in packed)
    assert not any(k.endswith(formats.PACKED_VALUES) for k in packed)
    loaded = copy.deepcopy(fresh)
    formats.load_packed_48(loaded, packed)
    assert sum(isinstance(m, Linear48) for m in loaded.modules()) == len(masks)
    assert torch.equal(_invariant_forward(loaded, batch).view(torch.int32), want.view(torch.int32))
    live = loaded.state_dict()
    assert live.keys() == packed.keys() == packed_live.keys()
    for k in packed:
        assert torch.equal(live[k], packed[k]) and torch.equal(live[k], packed_live[k]), k
    again = formats.pack_state_dict_48(formats.unpack_state_dict_48(live))
    assert again.keys() == live.keys() and all(torch.equal(again[k], live[k]) for k in live)
    bad = dict(packed)
    key = next(k for k in bad if k.endswith(formats.PACKED_META_48))
    bad[key] = torch.zeros_like(bad[key])
    with pytest.raises(ValueError, match="never writes"):
        formats.load_packed_48(copy.deepcopy(fresh), bad)

    # ---- the reference's reload keeps the zeros and drops the masks: from_zeros
    reloaded = copy.deepcopy(fresh)
    for m in reloaded.modules():
        if torch.is_tensor(getattr(m, "mask", None)):
            del m.mask
    assert pack_model_48_(reloaded) == []
    got_names = pack_model_48_(reloaded, from_zeros=True)
    assert set(masks) <= set(got_names)
    assert torch.equal(_invariant_forward(reloaded, batch).view(torch.int32), want.view(torch.int32))


def test_fp32_and_unstructured_linears_are_left_alone():
    import torch.nn as nn
    from vlmc.packed48 import pack_model_48_
    model = nn.ModuleDict(dict(a=nn.Linear(64, 32), b=nn.Linear(64, 32).to(torch.bfloat16), c=nn.Linear(64, 32).to(torch.bfloat16))).to(DEV)
    four = [True, True, True, False, False, True, False, False]
    model["a"].mask = torch.tensor(four, device=DEV).repeat(32, 8)                                  # fp32: not packed
    model["b"].mask = torch.rand(32, 64, device=DEV) > 0.5                                          # not 4:8
    assert pack_model_48_(model) == [] and all(type(m) is nn.Linear for m in model.values())
    model["c"].mask = torch.tensor(four[::-1], device=DEV).repeat(32, 8)
    assert pack_model_48_(model) == ["c"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_merged_sparse_lora_linear_converts(dtype):
    from lavis.peft.src.peft.tuners.lora import Linear as LoraLinear
    from vlmc import ops
    from vlmc.packed48 import Linear48, pack_model_48_
    gen = torch.Generator(device=DEV).manual_seed(3)
    holder = torch.nn.Module()
    holder.lin = LoraLinear(64, 48, r=4, lora_alpha=8, bias=True, merge_weights=False).to(DEV)
    lin = holder.lin
    lin.sparse = True
    with torch.no_grad():
        lin.weight.copy_(torch.randn(48, 64, generator=gen, device=DEV) * 0.05)
        lin.lora_B.weight.copy_(torch.randn(48, 4, generator=gen, device=DEV) * 0.05)
    lin.weight.data, lin.bias.data = lin.weight.data.to(dtype), lin.bias.data.to(dtype)      # (the LoRA factors stay fp32 parameters)
    keep, _ = ops.wanda_select(lin.weight.data, torch.ones(64, device=DEV), "nm", n=4, m=8)
    lin.mask = keep
    assert pack_model_48_(holder) == []                                        # a live adapter: not packable
    lin.merge()
    W, bias = lin.weight.data.clone(), lin.bias.data.clone()
    assert pack_model_48_(holder) == ["lin"] and isinstance(holder.lin, Linear48)
    x = torch.randn(9, 64, generator=gen, device=DEV).to(dtype)
    with torch.no_grad():
        assert _same(holder.lin(x, False), ops.linear_fwd(x, W * keep.to(dtype), bias))
